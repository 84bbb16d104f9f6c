"""GPU tests of the C entries of csrc/rcm.hip ON THEIR OWN, through the C ABI (``hp._capi``), on inputs and states ``hp.rcm`` never
builds: one block of a row partition at a time with its ghost columns, both index widths, ``index_base`` 0 and 1, rows in any
stored order, doubled neighbour lists, single levels made by hand, every launch of the walk entered from the state the
restatement says it has, and the one-workgroup kernel resumed in the middle of a walk with any admissible cursor.

1. graph count / fill: blocks of three cases in 1, 3 and 8 row ranges, sorted and shuffled, in the four forms; a repeated
   column, no stored diagonal, no rows, no graph entry; the row counts around the scan's blocks and its second-phase carry.
2. degrees with ``distinct`` 0 and 1 on those graphs, on E u E^T from the multigrid's symmetrise entries, on rows made by hand
   (lengths around the 8-lane group, repeats at distance 1, 8 and 9) and at row counts around a workgroup's end; init at the
   counts of neighbourless vertices around a workgroup.
3. one wide level, expand -> keys -> torch.sort -> number, after each launch: on every wide level of ``rc.rcm_trace`` and on
   levels made by hand; then the wide kernels alone walk whole graphs, every level.
4. the one-workgroup kernel: the record word for word, ``order`` and ``parent`` whole, from "first", resumed from every state
   the trace enters it with (``tree_then_narrow``: on a frontier of 10 that a wide level numbered), and resumed mid-walk
   with the trace's cursor, with z and with 0.
5. finish, the two bandwidths, the statuses of bad arguments (scalars and NULL pointers only: every call here hands the kernels
   indices inside their arrays, the kernels' range guards are not tested by making them necessary).

Expected values: tests/_rcm_cases.py restates each kernel in numpy with int64 throughout (tests/test_rcm_cases.py holds the
restatements against ``block_graph``, ``rcm_levels`` and the queue algorithm).  Everything is an integer: every comparison is
array_equal and no tolerance appears.  Every output buffer has one word more than it needs, holding BEHIND, which is asserted
intact after every launch; ``work`` holds exactly the words ``hpcla_rcm_work_bytes`` asks for and that word.

Which slip which test catches (argued from csrc/rcm.hip, not from runs of broken kernels):
  a dropped ``- base`` in count, fill or the      the base-1 forms of test_graph_of_every_block, of the row-count edges and of
  matrix bandwidth                                test_matrix_bandwidth_of_every_block: another row's entries or another column id
  ``c <= nrows`` for ``c < nrows``                the first ghost column behind a block is row_start + nrows in every cut block and
                                                  at every row-count edge: one entry too many in the last row
  g_rowptr[nrows] unwritten, or the scan carry    test_graph_at_the_row_count_edges: g_rowptr and info start as BEHIND; nrows =
  lost                                            1025, 2049, 262 145 open a scan block with the last row; block 256 needs the carry
  stored order not kept by the fill               the shuffled blocks and the repeated column, compared in stored order
  ``e2 <= e``, or a repeat test within a lane,    test_degrees_of_rows_made_by_hand: a repeat at distance 8 is met by the same lane
  in the degree kernel                            one trip later, at distance 1 and 9 by another lane; the one-value row
  a lane group split by the ``live`` edge         nrows = 31, 32, 33 and 8193 of the degrees; frontiers of 31, 32, 33 groups
  ``chunk < gridDim.y`` for the stride loop       ``star_chunk_wrap``: chunk 1024 holds 1 entry: a leaf never claimed (and 255 more
                                                  for a wrong e0), count and parent differ
  the ``__any`` exit taken by a lane's own        the hand-made levels mix rows of 1 .. 513 entries in one wave: a short row's group
  ``valid``, not the wave's                       sits beside a long one's
  a claim test other than ``== RCM_UNVISITED``    the 5 000-on-100 level and ``nonsymmetric_wide``: a vertex twice in ``cand`` (or never)
  an append position taken per lane without the   ``cand[:count]`` sorted must be the claimed set exactly: a hole leaves BEHIND inside,
  ballot's prefix                                 a collision loses a vertex
  ``cursor += RCM_NARROW_THREADS`` off by one     ``path1024_k6`` / ``path1025_k6``: the second start is the last lane of the first
                                                  sweep / the first lane of the second; a skipped position ends in status 2
  a resumed launch that trusts ``s_front``        the resumed states: LDS holds nothing of the earlier launch, the first level is wrong
  a cursor taken as exact, not as a bound         the mid-walk states entered with z and with 0
  ``lo + a`` replaced by ``a`` in the narrow      the parents after any second level, compared whole
  claim
  a level half done before the cap is noticed     the ``_plus1`` cases from "first": parent is compared whole at status 1
  ``order[nrows - i]`` in finish                  n = 1 (and every other n): p[0] is read behind the array
  the block maximum of wave 0 only                the graph whose only long edge sits in the last rows of the last workgroup
"""
import numpy as np
import pytest

from tests import _rcm_cases as rc
from tests.test_gpu_precond_kernels import FORM_IDS, FORMS, _call, _dev, _full, _host, _same, _status, _torch

pytestmark = pytest.mark.gpu

I64, I32 = np.int64, np.int32
BEHIND = rc.FREE                                                 # the word behind every output, and every place not yet written
INVALID, UNSUPPORTED = -1, -5                                    # HPCLA_ERR_INVALID, HPCLA_ERR_UNSUPPORTED of include/hpcla_rocm.h
ROW_EDGES = (1, 2, 1023, 1024, 1025, 2048, 2049, 262144, 262145, 262146)
_ON_DEVICE = {}


def _cuts(n, k):
    return [(n * j) // k for j in range(k + 1)]


def _padded(a, dtype):
    """A host array on the device with BEHIND behind it."""
    return _dev(np.concatenate([np.asarray(a, dtype=I64), [BEHIND]]), dtype)


# ---- 1. the graph ---------------------------------------------------------------------------------------------------------------------
def _graph(hp, split, n, row_start, form, tag):
    """count and fill on rows that already carry the form's base and type; returns the host graph and its device arrays."""
    sfx, Ti, base = form
    rowptr, colval, ci = split
    d_rowptr, d_colval, d_ci = _dev(rowptr, Ti), _dev(colval, Ti), _dev(ci, I64)
    words = hp._capi.load().hpcla_rcm_work_bytes(n) // 8
    work = _full(words + 1, BEHIND, I64)
    g_rowptr, info = _full(n + 2, BEHIND, I64), _full(2, BEHIND, I64)
    _call(hp, f"hpcla_rcm_graph_count_{sfx}", d_rowptr, d_colval, d_ci, n, row_start, base, g_rowptr, info, work, None)
    gp = _host(g_rowptr)
    nnz = int(gp[n])
    assert int(_host(work)[words]) == BEHIND, (tag, "the word behind work")
    assert gp[n + 1] == BEHIND and _host(info).tolist() == [nnz, BEHIND], (tag, "count", gp[n:].tolist(), _host(info).tolist())
    g_cols = _full(nnz + 1, BEHIND, I32)
    _call(hp, f"hpcla_rcm_graph_fill_{sfx}", d_rowptr, d_colval, d_ci, n, row_start, base, g_rowptr, g_cols, None)
    gc = _host(g_cols)
    assert gc[nnz] == BEHIND, (tag, "the word behind g_cols")
    _same(_host(g_rowptr), gp, (tag, "g_rowptr after the fill"))
    return gp[:n + 1], gc[:nnz].astype(I64), (g_rowptr, g_cols)


def _check_graph(hp, split0, n, row_start, form, tag):
    """``split0``: 0-based int64 (rowptr, colval, col_indices); the form is put on here."""
    sfx, Ti, base = form
    split = ((split0[0] + base).astype(Ti), (split0[1] + base).astype(Ti), np.asarray(split0[2], dtype=I64) + base)
    want = rc.graph_of_block(*split, n, row_start, base)
    gp, gc, dev = _graph(hp, split, n, row_start, form, tag)
    _same(gp, want[0], (tag, "g_rowptr"))
    _same(gc, want[1], (tag, "g_cols"))
    return gp, gc, dev


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", ["grid33x31", "delaunay2000", "nonsymmetric"])
def test_graph_of_every_block(hp, name, form):
    """Sorted rows against ``block_graph`` as well; shuffled rows in their stored order; then the degrees of each graph."""
    A = rc.matrix(name)
    n = A.shape[0]
    sfx, Ti, base = form
    for k in (1, 3, 8):
        cuts = _cuts(n, k)
        for j in range(k):
            lo, hi = cuts[j], cuts[j + 1]
            tag = (name, k, j, sfx, base)
            split = rc.split_block(A, lo, hi, base, Ti)
            gp, gc, dev = _graph(hp, split, hi - lo, lo, form, tag)
            want = rc.block_graph(A, lo, hi)
            _same(gp, want[0], (tag, "g_rowptr"))
            _same(gc, want[1], (tag, "g_cols"))
            shuffled = rc.split_block(A, lo, hi, base, Ti, shuffle_seed=7 * k + j)
            sp_, sc, sdev = _graph(hp, shuffled, hi - lo, lo, form, tag + ("shuffled",))
            swant = rc.graph_of_block(*shuffled, hi - lo, lo, base)
            _same(sp_, swant[0], (tag, "shuffled g_rowptr"))
            _same(sc, swant[1], (tag, "shuffled g_cols: stored order"))
            for distinct in (0, 1):
                _check_degrees(hp, sdev, (sp_, sc), hi - lo, distinct, tag + ("shuffled",))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_graph_of_rows_made_by_hand(hp, form):
    # rows 20 .. 23 of a matrix with 30 columns; columns 19 and 24 are the ghosts next to the block on either side
    ci = np.array([3, 19, 20, 21, 22, 23, 24, 29])
    rows = [[21, 29, 21, 20, 3, 21],                              # 21 stored three times, the diagonal in the middle
            [24, 19],                                             # ghosts only, no diagonal: an empty row
            [23, 20, 23],                                         # no stored diagonal, a column twice
            [23]]                                                 # the diagonal alone
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    colval = np.searchsorted(ci, np.concatenate(rows))
    gp, gc, _ = _check_graph(hp, (rowptr, colval, ci), 4, 20, form, ("by hand", form[0], form[2]))
    assert gp.tolist() == [0, 3, 3, 6, 6] and gc.tolist() == [1, 1, 1, 3, 0, 3]
    # a block whose graph has no entry: diagonal and ghosts only
    rows = [[3, 20], [21], [29, 22, 24], [19, 23]]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    gp, gc, dev = _check_graph(hp, (rowptr, np.searchsorted(ci, np.concatenate(rows)), ci), 4, 20, form, ("no entry", form[0]))
    assert gp.tolist() == [0] * 5 and len(gc) == 0
    for distinct in (0, 1):
        deg = _full(5, BEHIND, I32)
        _call(hp, "hpcla_rcm_degrees", dev[0], None, 4, distinct, deg, None)          # g_cols NULL downstream
        assert _host(deg).tolist() == [0, 0, 0, 0, BEHIND]
    # no rows
    sfx, Ti, base = form
    g_rowptr, info, work = _full(2, BEHIND, I64), _full(2, BEHIND, I64), _full(3, BEHIND, I64)
    _call(hp, f"hpcla_rcm_graph_count_{sfx}", None, None, None, 0, 9, base, g_rowptr, info, work, None)
    _call(hp, f"hpcla_rcm_graph_fill_{sfx}", None, None, None, 0, 9, base, g_rowptr, None, None)
    assert _host(g_rowptr).tolist() == [0, BEHIND] and _host(info).tolist() == [0, BEHIND] and _host(work).tolist() == [BEHIND] * 3


def _band_rows(n, row_start):
    """Row i stores the global columns row_start + i - 1, + i, + i + 1: the first and the last row reach the ghost next to the
    block.  0-based (rowptr, colval, col_indices)."""
    ci = np.arange(row_start - 1, row_start + n + 1, dtype=I64)
    colval = (np.arange(n, dtype=I64)[:, None] + np.arange(3, dtype=I64)[None, :]).ravel()
    return 3 * np.arange(n + 1, dtype=I64), colval, ci


@pytest.mark.parametrize("n", ROW_EDGES)
def test_graph_at_the_row_count_edges(hp, n):
    split = _band_rows(n, 5)
    for form in FORMS:
        gp, gc, _ = _check_graph(hp, split, n, 5, form, (n, form[0], form[2]))
        assert int(gp[n]) == 2 * (n - 1) == len(gc)
        if n > 262144:
            assert int(gp[262144]) == 2 * 262144 - 1                          # the offset of scan block 256: the carry


# ---- 2. degrees and init ----------------------------------------------------------------------------------------------------------------
def _check_degrees(hp, dev, g, n, distinct, tag):
    deg = _full(n + 1, BEHIND, I32)
    _call(hp, "hpcla_rcm_degrees", dev[0], dev[1], n, distinct, deg, None)
    got = _host(deg)
    assert got[n] == BEHIND, (tag, "the word behind deg")
    _same(got[:n].astype(I64), rc.degrees_of(g[0], g[1], distinct), (tag, "deg", distinct))
    return got[:n]


def _rows_on_device(rows, n):
    gp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(I64)
    gc = np.concatenate([np.asarray(r, dtype=I64) for r in rows]) if gp[-1] else np.zeros(0, dtype=I64)
    assert len(rows) == n and (len(gc) == 0 or (gc.min() >= 0 and gc.max() < n))
    return (gp, gc), (_dev(gp, I64), _padded(gc, I32))


def test_degrees_of_rows_made_by_hand(hp):
    rng = np.random.default_rng(41)
    n = 5000
    rows = []
    for length in (0, 1, 7, 8, 9, 16, 17, 4096):
        base_row = rng.permutation(n)[:length]
        rows.append(base_row)
        for dist in (1, 8, 9):
            if length > dist:
                for pos in (0, length - dist - 1):                  # the pair at the row's head and at its tail
                    r = base_row.copy()
                    r[pos + dist] = r[pos]
                    rows.append(r)
        if length:
            rows.append(np.full(length, base_row[0]))               # one value only
    want_some = {len(rows) - 1: 1, 0: 0}
    rows += [np.zeros(0, dtype=I64)] * (n - len(rows))
    g, dev = _rows_on_device(rows, n)
    assert int(np.diff(g[0]).max()) == 4096
    got = _check_degrees(hp, dev, g, n, 1, "by hand")
    for i, d in want_some.items():
        assert got[i] == d
    _check_degrees(hp, dev, g, n, 0, "by hand")


@pytest.mark.parametrize("n", [31, 32, 33, 8193])
def test_degrees_around_a_workgroups_end(hp, n):
    rng = np.random.default_rng(n)
    rows = [rng.integers(0, min(n, 12), rng.integers(0, 21)) for _ in range(n)]
    rows[n - 1] = np.array([0, 1, 0, 2, 1, 0, 3, 3, 4, 0])         # the last row has entries: 5 distinct
    g, dev = _rows_on_device(rows, n)
    assert _check_degrees(hp, dev, g, n, 1, n)[n - 1] == 5
    assert _check_degrees(hp, dev, g, n, 0, n)[n - 1] == 10


def test_degrees_of_the_doubled_graph(hp):
    """E u E^T of ``nonsymmetric_wide`` through the symmetrise entries, as rcm.py chains them: the distinct degrees are those of
    the set union whatever order the in-lists took, the plain ones the stored lengths."""
    lib = hp._capi.load()
    indptr, indices = rc.block_graph(rc.matrix("nonsymmetric_wide"))
    n = len(indptr) - 1
    s_rowptr, s_cols = _dev(indptr, I64), _dev(indices, I32)
    work = _full(lib.hpcla_amg_work_bytes(n) // 8, 0, I64)
    indeg, u_rowptr, info = _full(n, BEHIND, I64), _full(n + 2, BEHIND, I64), _full(2, BEHIND, I64)
    _call(hp, "hpcla_amg_symmetrise_count", s_rowptr, s_cols, n, indeg, u_rowptr, info, work, None)
    d_ptr, d_cols = rc.doubled_graph(indptr, indices)
    _same(_host(u_rowptr)[:n + 1], d_ptr, "u_rowptr")
    u_cols = _full(int(d_ptr[-1]) + 1, BEHIND, I32)
    _call(hp, "hpcla_amg_symmetrise_fill", s_rowptr, s_cols, n, u_rowptr, indeg, u_cols, None)
    got_cols = _host(u_cols)[:-1].astype(I64)
    rows = np.repeat(np.arange(n), np.diff(d_ptr))
    _same(got_cols[np.lexsort((got_cols, rows))], d_cols[np.lexsort((d_cols, rows))], "u_cols, each row sorted")
    want = np.diff(rc.block_graph(rc.matrix("nonsymmetric_wide"), symmetric=False)[0])
    got = _check_degrees(hp, (u_rowptr, u_cols), (d_ptr, got_cols), n, 1, "doubled")
    _same(got.astype(I64), want, "the distinct degrees are those of the set union")
    _check_degrees(hp, (u_rowptr, u_cols), (d_ptr, got_cols), n, 0, "doubled")
    assert int((np.diff(d_ptr) > 8).sum()) >= 1000 and int((np.diff(d_ptr) - want).sum()) >= 1000


def test_degrees_of_the_longest_row(hp):
    """``star_chunk_wrap`` with distinct = 0 only (the distinct count is quadratic in a row)."""
    d = _on_device("star_chunk_wrap")
    got = _check_degrees(hp, (d["gp"], d["gc"]), d["g"], d["n"], 0, "star_chunk_wrap")
    assert int(got.max()) == 1024 * 256 + 1


@pytest.mark.parametrize("z", [0, 1, 255, 256, 257, 600])
def test_init(hp, z):
    n = 600
    rng = np.random.default_rng(z)
    deg = rng.integers(1, 6, n)
    deg[rng.permutation(n)[:z]] = 0
    by = np.lexsort((np.arange(n), deg))
    rank, parent, order, info = _full(n + 1, BEHIND, I32), _full(n + 1, BEHIND, I32), _full(n + 1, BEHIND, I32), _full(2, BEHIND, I64)
    _call(hp, "hpcla_rcm_init", _dev(deg, I32), _dev(by, I32), n, rank, parent, order, info, None)
    w_rank, w_parent, w_head, w_z = rc.init_of(deg, by)
    assert w_z == z and _host(info).tolist() == [z, BEHIND]
    _same(_host(rank).astype(I64), np.concatenate([w_rank, [BEHIND]]), (z, "rank"))
    _same(_host(parent).astype(I64), np.concatenate([w_parent, [BEHIND]]), (z, "parent"))
    _same(_host(order).astype(I64), np.concatenate([w_head, np.full(n + 1 - z, BEHIND)]), (z, "order: [:z] numbered, the rest as given"))


# ---- 3. a wide level --------------------------------------------------------------------------------------------------------------------
def _on_device(name, doubled=False):
    """The case's graph, by_degree and rank on the device, with its trace; once per session."""
    key = (name, doubled)
    if key not in _ON_DEVICE:
        trace, g = rc.traced(name, doubled)
        n = len(g[0]) - 1
        c = trace[0]
        _ON_DEVICE[key] = dict(n=n, g=g, trace=trace, gp=_dev(g[0], I64), gc=_padded(g[1], I32) if len(g[1]) else None,
                               by=_dev(c["by_degree"], I32), rank=_dev(c["rank"], I32), by_host=c["by_degree"], rank_host=c["rank"],
                               z=c["z"], longest=int(np.diff(g[0]).max()))
    return _ON_DEVICE[key]


def _wide_level(hp, d, parent, order, lo, hi, tag, longest=None):
    """expand, keys, torch.sort and number on the level order[lo .. hi) of the graph ``d``; everything the issue lists is compared
    after each launch.  Returns (parent, order, the claimed set) as the device left them."""
    torch = _torch()
    n, g = d["n"], d["g"]
    parent, order = np.asarray(parent, dtype=I64), np.asarray(order, dtype=I64)
    d_parent, d_order = _padded(parent, I32), _padded(order, I32)
    cand, count = _full(n + 1, BEHIND, I32), _full(2, BEHIND, I64)
    _call(hp, "hpcla_rcm_expand", d["gp"], d["gc"], n, d_order, lo, hi, d["longest"] if longest is None else longest, d_parent,
          cand, count, None)
    want_parent, want_set = rc.expand_of(*g, parent, order, lo, hi)
    ncand = len(want_set)
    assert _host(count).tolist() == [ncand, BEHIND], (tag, "count", _host(count).tolist(), ncand)
    got_cand = _host(cand).astype(I64)
    _same(np.sort(got_cand[:ncand]), want_set, (tag, "cand as a sorted set: every claimed vertex once"))
    assert np.all(got_cand[ncand:] == BEHIND), (tag, "cand behind count")
    _same(_host(d_parent).astype(I64), np.concatenate([want_parent, [BEHIND]]), (tag, "parent"))
    _same(_host(d_order).astype(I64), np.concatenate([order, [BEHIND]]), (tag, "order after the expand"))
    want_order = order.copy()
    if ncand:
        keys = _full(n + 1, BEHIND, I64)
        _call(hp, "hpcla_rcm_keys", cand, ncand, n, d_parent, d["rank"], keys, None)
        got_keys = _host(keys)
        _same(got_keys[:ncand], rc.keys_of(got_cand[:ncand], want_parent, d["rank_host"]), (tag, "keys of the cand the device wrote"))
        assert np.all(got_keys[ncand:] == BEHIND), (tag, "keys behind ncand")
        ordered = torch.sort(keys[:ncand]).values
        _call(hp, "hpcla_rcm_number", ordered, ncand, n, d["by"], hi, d_order, None)
        want_order[hi:hi + ncand] = rc.number_of(np.sort(rc.keys_of(want_set, want_parent, d["rank_host"])), d["by_host"])
        _same(_host(d_order).astype(I64), np.concatenate([want_order, [BEHIND]]), (tag, "order[hi : hi + ncand], the rest untouched"))
        _same(_host(d_parent).astype(I64), np.concatenate([want_parent, [BEHIND]]), (tag, "parent after keys and number"))
    return want_parent, want_order, want_set


@pytest.mark.parametrize("name", ["star_cap_plus1", "tree_frontier_cap_plus1", "degree_sum_cap_plus1", "random20000", "star_chunk_wrap",
                                  "nonsymmetric_wide", "tree_then_narrow"])
def test_every_wide_level_of_the_trace(hp, name):
    d = _on_device(name, doubled=name == "nonsymmetric_wide")
    wide = [t for t in d["trace"] if t["kind"] == "wide"]
    assert len(wide) >= 1
    for k, t in enumerate(wide):
        parent, order, claimed = _wide_level(hp, d, t["parent"], t["order"], t["lo"], t["hi"], (name, "wide level", k))
        assert np.array_equal(parent, t["parent_after"]) and np.array_equal(order, t["order_after"]) and np.array_equal(claimed, t["cand"])
    if name == "star_chunk_wrap":
        # the centre lists 1024 * 256 + 1 leaves, the start among them; the one entry of chunk 1024 is a leaf still to be claimed
        assert [len(t["cand"]) for t in wide] == [1024 * 256, 0] and d["longest"] == 1024 * 256 + 1
        centre = wide[0]["order"][wide[0]["lo"]]
        assert wide[0]["hi"] - wide[0]["lo"] == 1 and wide[0]["parent"][d["g"][1][d["g"][0][centre + 1] - 1]] == rc.UNVISITED
    if name == "nonsymmetric_wide":
        assert len(wide) > 1 and int(d["g"][0][-1]) - int(d["trace"][0]["deg"].sum()) >= 1000      # repeated neighbours


def _level_by_hand(f, lengths, seed, fresh=2000, numbered=50, targets=None):
    """A level made by hand: ``numbered`` vertices hold the numbers below lo, ``f`` frontier vertices the numbers lo .. hi - 1,
    all with a parent below lo; the ``fresh`` others are unvisited.  The k-th vertex from the frontier on lists
    ``lengths[k % len(lengths)]`` vertices drawn from ``targets`` (default: all, so numbered, frontier and fresh ones), repeats
    allowed; the fresh vertices have rows too, for the level after."""
    rng = np.random.default_rng(seed)
    n = numbered + f + fresh
    perm = rng.permutation(n)
    lo, hi = numbered, numbered + f
    order = np.full(n, BEHIND, dtype=I64)
    order[:hi] = perm[:hi]
    parent = np.full(n, rc.UNVISITED, dtype=I64)
    parent[perm[:hi]] = rng.integers(0, lo, hi)
    pool = np.arange(n) if targets is None else targets(perm, lo, hi)
    rows = [np.zeros(0, dtype=I64)] * n
    for k in range(n - lo):
        rows[perm[lo + k]] = pool[rng.integers(0, len(pool), lengths[k % len(lengths)])]
    return _level_on_device(rows, n, rng), parent, order, lo, hi


def _level_on_device(rows, n, rng):
    g, (gp, gc) = _rows_on_device(rows, n)
    by = rng.permutation(n)                                         # any permutation serves as by_degree here
    rank = np.empty(n, dtype=I64)
    rank[by] = np.arange(n)
    return dict(n=n, g=g, gp=gp, gc=gc, by=_dev(by, I32), rank=_dev(rank, I32), by_host=by, rank_host=rank,
                longest=int(np.diff(g[0]).max()))


MIXED = (1, 7, 8, 9, 255, 256, 257, 513)


@pytest.mark.parametrize("f", [1, 31, 32, 33, 5000])
def test_a_level_made_by_hand(hp, f):
    lengths = (513,) if f == 1 else MIXED
    d, parent, order, lo, hi = _level_by_hand(f, lengths, f)
    assert d["longest"] == 513 and hi - lo == f
    first = _wide_level(hp, d, parent, order, lo, hi, ("by hand", f))
    assert len(first[2]) > 0
    # longest_row larger than any row: more chunks, which find nothing
    again = _wide_level(hp, d, parent, order, lo, hi, ("by hand", f, "longest_row too large"), longest=3 * 513 + 1000)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    # the next level on the state this one left (parents at and above lo now exist)
    _wide_level(hp, d, first[0], first[1], hi, hi + len(first[2]), ("by hand", f, "the level after"))


def test_many_waves_claim_the_same_few_vertices(hp):
    """5 000 frontier vertices that all list the same 100 fresh vertices, each row rotated by its number: 100 candidates, each
    with the smallest lister's number, which is lo."""
    rng = np.random.default_rng(5)
    n, lo, hi = 5200, 50, 5050
    perm = rng.permutation(n)
    order = np.full(n, BEHIND, dtype=I64)
    order[:hi] = perm[:hi]
    parent = np.full(n, rc.UNVISITED, dtype=I64)
    parent[perm[:hi]] = rng.integers(0, lo, hi)
    fresh = perm[hi:hi + 100]
    rows = [np.zeros(0, dtype=I64)] * n
    for k in range(hi - lo):
        rows[perm[lo + k]] = np.roll(fresh, k)
    d = _level_on_device(rows, n, rng)
    got_parent, got_order, claimed = _wide_level(hp, d, parent, order, lo, hi, "5000 on 100")
    assert len(claimed) == 100 and np.all(got_parent[claimed] == lo) and np.array_equal(claimed, np.sort(fresh))


def test_a_level_whose_neighbours_are_all_numbered(hp):
    numbered_only = lambda perm, lo, hi: perm[:hi]
    d, parent, order, lo, hi = _level_by_hand(700, MIXED, 9, targets=numbered_only)
    got_parent, got_order, claimed = _wide_level(hp, d, parent, order, lo, hi, "all numbered")
    assert len(claimed) == 0 and np.array_equal(got_parent, parent) and np.array_equal(got_order, order)


def test_an_empty_level_resets_the_count_and_nothing_else(hp):
    d, parent, order, lo, hi = _level_by_hand(33, MIXED, 3)
    for a, b, longest in ((hi, hi, d["longest"]), (lo, hi, 0), (0, 0, 0)):
        d_parent, d_order = _padded(parent, I32), _padded(order, I32)
        cand, count = _full(d["n"] + 1, BEHIND, I32), _full(2, BEHIND, I64)
        _call(hp, "hpcla_rcm_expand", d["gp"], d["gc"], d["n"], d_order, a, b, longest, d_parent, cand, count, None)
        assert _host(count).tolist() == [0, BEHIND] and np.all(_host(cand) == BEHIND)
        _same(_host(d_parent).astype(I64), np.concatenate([parent, [BEHIND]]), "parent")
        _same(_host(d_order).astype(I64), np.concatenate([order, [BEHIND]]), "order")


@pytest.mark.parametrize("name", ["grid33x31", "components9", "delaunay2000", "nonsymmetric"])
def test_the_wide_kernels_walk_a_whole_graph(hp, name):
    """Every level by expand / keys / sort / number, each start made on the host: the numbers the one-workgroup kernel gives."""
    torch = _torch()
    d = _on_device(name, doubled=name == "nonsymmetric")
    n, trace = d["n"], d["trace"]
    final = trace[-1]
    d_parent, d_order = _padded(trace[0]["parent"], I32), _padded(trace[0]["order"], I32)
    cand, keys, count = _full(n + 1, BEHIND, I32), _full(n + 1, BEHIND, I64), _full(2, BEHIND, I64)
    lo = hi = d["z"]
    levels = 0
    while hi < n or lo < hi:
        if lo == hi:                                                # the next start, as the trace numbers it
            s = int(final["order_after"][hi])
            d_parent[s] = hi
            d_order[hi] = s
            lo, hi = hi, hi + 1
            levels += 1
        _call(hp, "hpcla_rcm_expand", d["gp"], d["gc"], n, d_order, lo, hi, d["longest"], d_parent, cand, count, None)
        ncand = int(count[0].item())
        assert 0 <= ncand <= n - hi, (name, lo, hi, ncand)
        if ncand == 0:
            lo = hi
            continue
        _call(hp, "hpcla_rcm_keys", cand, ncand, n, d_parent, d["rank"], keys, None)
        _call(hp, "hpcla_rcm_number", torch.sort(keys[:ncand]).values, ncand, n, d["by"], hi, d_order, None)
        lo, hi = hi, hi + ncand
        levels += 1
    assert levels < 200 and levels == rc.trace_facts(trace, n)["levels"], (name, levels)
    _same(_host(d_order).astype(I64), np.concatenate([final["order_after"], [BEHIND]]), (name, "order"))
    _same(_host(d_parent).astype(I64), np.concatenate([final["parent_after"], [BEHIND]]), (name, "parent"))
    assert int(_host(count)[1]) == BEHIND and int(_host(cand)[n]) == BEHIND and int(_host(keys)[n]) == BEHIND
    if name == "nonsymmetric":
        assert np.array_equal(final["order_after"][::-1], rc.expected(name, False)[0])


# ---- 4. the one-workgroup kernel ------------------------------------------------------------------------------------------------------
def _narrow(hp, d, parent, order, lo, hi, cursor, first, tag):
    """One launch; returns (record, parent, order) with the words behind them checked."""
    d_parent, d_order, record = _padded(parent, I32), _padded(order, I32), _full(7, BEHIND, I64)
    z_dev = _dev([d["z"]], I64) if first else None
    _call(hp, "hpcla_rcm_narrow", d["gp"], d["gc"], d["by"], d["rank"], d["n"], lo, hi, cursor, z_dev, d_parent, d_order, record, None)
    rec, got_parent, got_order = _host(record), _host(d_parent).astype(I64), _host(d_order).astype(I64)
    assert rec[6] == BEHIND and got_parent[-1] == BEHIND and got_order[-1] == BEHIND, (tag, "a word behind")
    return tuple(int(v) for v in rec[:6]), got_parent[:-1], got_order[:-1]


def _check_launch(hp, d, t, tag, first=None):
    first = t["first"] if first is None else first
    args = (0, 0, 0) if first else (t["lo"], t["hi"], t["cursor"])
    rec, parent, order = _narrow(hp, d, t["parent"], t["order"], *args, first, tag)
    assert rec == tuple(t["record"]), (tag, "record", rec, t["record"])
    _same(order, t["order_after"], (tag, "order"))
    _same(parent, t["parent_after"], (tag, "parent"))


@pytest.mark.parametrize("name", ["path1", "path2", "path300", "pairs500", "components9", "path1024_k6", "path1025_k6", "path3000_k6",
                                  "star_cap", "tree_frontier_cap", "degree_sum_cap", "star_cap_plus1", "tree_frontier_cap_plus1",
                                  "degree_sum_cap_plus1"])
def test_the_first_launch(hp, name):
    d = _on_device(name)
    t = d["trace"][0]
    assert t["kind"] == "narrow" and t["first"]
    _check_launch(hp, d, t, (name, "first"))
    if name.endswith("_plus1"):
        assert t["record"][3] == rc.WIDE                                       # a cap exceeded: parent compared whole above
        lo, hi = t["record"][:2]
        assert int((t["parent_after"] != rc.UNVISITED).sum()) == hi            # nothing claimed beyond the levels done
    elif name not in ("star_cap",):
        assert t["record"][3] == rc.DONE and len(d["trace"]) == 1
    if name.endswith("_k6"):
        length = int(name[4:-3])
        assert t["record"] == (length + 6, length + 6, length + 1, rc.DONE, length + 2, 2)


@pytest.mark.parametrize("name", ["star_cap_plus1", "tree_frontier_cap_plus1", "random20000", "nonsymmetric_wide", "tree_then_narrow"])
def test_resumed_from_every_state_of_the_trace(hp, name):
    d = _on_device(name, doubled=name == "nonsymmetric_wide")
    launches = [t for t in d["trace"] if t["kind"] == "narrow"]
    assert len(launches) >= 2 and launches[0]["first"]
    for k, t in enumerate(launches):
        _check_launch(hp, d, t, (name, "launch", k))
        if t["first"]:                                                         # "first" is lo = hi = cursor = z and nothing else
            assert t["lo"] == t["hi"] == t["cursor"] == d["z"]
            _check_launch(hp, d, t, (name, "launch", k, "z by value"), first=False)
    if name == "tree_then_narrow":                                             # the frontier of 10 was numbered by the wide level
        t = launches[1]
        assert t["hi"] - t["lo"] == 10 and t["record"][3:] == (rc.DONE, 1, 0) and t["record"][0] == d["n"]


@pytest.mark.parametrize("name", ["grid33x31", "components9"])
def test_resumed_in_the_middle_of_a_walk(hp, name):
    """At level boundaries and at component boundaries (lo == hi), with the trace's cursor, with z and with 0: a cursor is a
    position to scan from, so all three give the same order, and the same record wherever a start is still to be found."""
    d = _on_device(name)
    n, z = d["n"], d["z"]
    assert len(d["trace"]) == 1
    final = d["trace"][0]
    marks = final["marks"]
    ends = [m for m in marks if m[0] == m[1]]
    inner = [m for m in marks if m[0] < m[1]]
    assert len(ends) == (3 if name == "components9" else 2) and ends[0][:3] == (z, z, z) and ends[-1][:2] == (n, n)
    total_levels, total_starts, last_cursor = final["record"][4], final["record"][5], final["record"][2]
    for lo, hi, cursor, levels, starts in ends + [inner[1], inner[len(inner) // 2], inner[-1]]:
        parent, order = rc.state_at(final, lo, hi)
        for given in dict.fromkeys((cursor, z, 0)):
            tag = (name, lo, hi, "cursor", given)
            rec, got_parent, got_order = _narrow(hp, d, parent, order, lo, hi, given, False, tag)
            left = total_starts - starts
            want = (n, n, last_cursor if left else given, rc.DONE, total_levels - levels, left)
            assert rec == want, (tag, "record", rec, want)
            _same(got_order, final["order_after"], (tag, "order"))
            _same(got_parent, final["parent_after"], (tag, "parent"))


def test_a_graph_without_edges(hp):
    n = 37
    by = np.arange(n)
    d = dict(n=n, z=n, gp=_dev(np.zeros(n + 1), I64), gc=None, by=_dev(by, I32), rank=_dev(by, I32))
    rec, parent, order = _narrow(hp, d, by, by, 0, 0, 0, True, "no edges")
    assert rec == (n, n, n, rc.DONE, 0, 0) and np.array_equal(parent, by) and np.array_equal(order, by)


# ---- 5. finish, the bandwidths, the statuses --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_finish(hp, n):
    order = np.random.default_rng(n).permutation(n)
    for row_start in (0, 2 ** 31 + 5):
        p, inv = _full(n + 1, BEHIND, I64), _full(n + 1, BEHIND, I32)
        _call(hp, "hpcla_rcm_finish", _padded(order, I32), n, row_start, p, inv, None)
        want_inv = np.empty(n, dtype=I64)
        want_inv[order[::-1]] = np.arange(n)
        _same(_host(p), np.concatenate([order[::-1] + row_start, [BEHIND]]), (n, row_start, "p"))
        _same(_host(inv).astype(I64), np.concatenate([want_inv, [BEHIND]]), (n, row_start, "inv"))


def _graph_bandwidth(hp, gp, gc, n, inv):
    out = _full(2, BEHIND, I64)
    _call(hp, "hpcla_rcm_graph_bandwidth", gp, gc, n, inv, out, None)
    got = _host(out).tolist()
    assert got[1] == BEHIND
    return got[0]


def test_graph_bandwidth(hp):
    for name in ("grid33x31", "delaunay2000", "components9"):
        d = _on_device(name)
        p = rc.expected(name)[0]
        inv = np.empty(d["n"], dtype=I64)
        inv[p] = np.arange(d["n"])
        assert _graph_bandwidth(hp, d["gp"], d["gc"], d["n"], None) == rc.bandwidth_of_graph(*d["g"])
        assert _graph_bandwidth(hp, d["gp"], d["gc"], d["n"], _dev(inv, I32)) == rc.bandwidth_of_graph(*d["g"], p) \
            == rc.expected(name)[1]["bandwidth_after"]
    # the only long edge in the last rows of the last workgroup (rows 512 .. 599), held by its last wave
    n = 600
    rows = [np.array([i + 1]) for i in range(n - 1)] + [np.array([3])]
    g, (gp, gc) = _rows_on_device(rows, n)
    assert _graph_bandwidth(hp, gp, gc, n, None) == n - 1 - 3 == rc.bandwidth_of_graph(*g)
    inv = np.arange(n)[::-1].copy()
    inv[[3, 300]] = inv[[300, 3]]
    want = int(np.abs(inv[np.repeat(np.arange(n), np.diff(g[0]))] - inv[g[1]]).max())
    assert _graph_bandwidth(hp, gp, gc, n, _dev(inv, I32)) == want == 299           # |inv[599] - inv[3]|
    # no edges: the output goes from BEHIND to 0
    assert _graph_bandwidth(hp, _dev(np.zeros(n + 1), I64), None, n, None) == 0
    assert _graph_bandwidth(hp, None, None, 0, None) == 0


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_matrix_bandwidth_of_every_block(hp, form):
    """max |global row - global column| over the rank's rows: ghost columns decide it in the cut blocks."""
    sfx, Ti, base = form
    for name in ("grid33x31", "delaunay2000", "nonsymmetric"):
        A = rc.matrix(name)
        n = A.shape[0]
        for k in (1, 3, 8):
            cuts = _cuts(n, k)
            for j in range(k):
                lo, hi = cuts[j], cuts[j + 1]
                C = A[lo:hi].tocoo()
                want = int(np.abs(C.row + lo - C.col).max())
                own = (C.col >= lo) & (C.col < hi)
                for seed in (None, j):
                    rowptr, colval, ci = rc.split_block(A, lo, hi, base, Ti, shuffle_seed=seed)
                    out = _full(2, BEHIND, I64)
                    _call(hp, f"hpcla_bandwidth_{sfx}", _dev(rowptr, Ti), _dev(colval, Ti), _dev(ci, I64), hi - lo, lo, base, out, None)
                    assert _host(out).tolist() == [want, BEHIND], (name, k, j, sfx, base, seed)
                if k == 8:
                    assert want > int(np.abs(C.row + lo - C.col)[own].max()), "a ghost column decides the maximum"
    out = _full(2, BEHIND, I64)
    _call(hp, f"hpcla_bandwidth_{sfx}", None, None, None, 0, 3, base, out, None)
    assert _host(out).tolist() == [0, BEHIND]


def test_the_caps_and_the_work_size(hp):
    lib = hp._capi.load()
    assert lib.hpcla_rcm_frontier_cap() == rc.FRONTIER_CAP and lib.hpcla_rcm_candidate_cap() == rc.CANDIDATE_CAP
    assert lib.hpcla_rcm_work_bytes(-1) < 0
    for n, blocks in ((0, 1), (1, 1), (1024, 1), (1025, 2), (262145, 257)):
        assert lib.hpcla_rcm_work_bytes(n) == 8 * (1 + blocks), n


def test_bad_arguments_return_a_status(hp):
    """Scalars and NULL pointers only: every call below is rejected before any launch."""
    a = _full(64, 0, I64)                                            # stands for every array: no call below reaches a kernel
    big = 2 ** 31 - 1

    def bad(want, name, good, **kw):
        args = dict(good, **kw)
        got = _status(hp, name, *args.values())
        assert got == want, (name, kw, got)
        assert hp._capi.last_error(), (name, kw)

    for sfx in ("i32", "i64"):
        good = dict(rowptr=a, colval=a, ci=a, nrows=4, row_start=0, base=0, g_rowptr=a, info=a, work=a, stream=None)
        for kw in (dict(nrows=-1), dict(base=2), dict(base=-1), dict(g_rowptr=None), dict(info=None), dict(work=None), dict(rowptr=None)):
            bad(INVALID, f"hpcla_rcm_graph_count_{sfx}", good, **kw)
        bad(UNSUPPORTED, f"hpcla_rcm_graph_count_{sfx}", good, nrows=big)
        good = dict(rowptr=a, colval=a, ci=a, nrows=4, row_start=0, base=0, g_rowptr=a, g_cols=a, stream=None)
        for kw in (dict(nrows=-1), dict(base=2), dict(base=-1), dict(rowptr=None), dict(g_rowptr=None)):
            bad(INVALID, f"hpcla_rcm_graph_fill_{sfx}", good, **kw)
        bad(UNSUPPORTED, f"hpcla_rcm_graph_fill_{sfx}", good, nrows=big)
        good = dict(rowptr=a, colval=a, ci=a, nrows=4, row_start=0, base=0, out=a, stream=None)
        for kw in (dict(nrows=-1), dict(base=2), dict(base=-1), dict(out=None), dict(rowptr=None)):
            bad(INVALID, f"hpcla_bandwidth_{sfx}", good, **kw)
    good = dict(g_rowptr=a, g_cols=a, nrows=4, distinct=1, deg=a, stream=None)
    for kw in (dict(nrows=-1), dict(g_rowptr=None), dict(deg=None)):
        bad(INVALID, "hpcla_rcm_degrees", good, **kw)
    bad(UNSUPPORTED, "hpcla_rcm_degrees", good, nrows=big)
    good = dict(deg=a, by=a, nrows=4, rank=a, parent=a, order=a, info=a, stream=None)
    for kw in (dict(nrows=-1), dict(info=None), dict(deg=None), dict(by=None), dict(rank=None), dict(parent=None), dict(order=None)):
        bad(INVALID, "hpcla_rcm_init", good, **kw)
    bad(UNSUPPORTED, "hpcla_rcm_init", good, nrows=big)
    good = dict(g_rowptr=a, g_cols=a, by=a, rank=a, nrows=4, lo=1, hi=2, cursor=1, first=None, parent=a, order=a, record=a, stream=None)
    for kw in (dict(nrows=-1), dict(lo=3), dict(lo=-1), dict(hi=5), dict(cursor=5), dict(cursor=-1), dict(record=None), dict(g_rowptr=None),
               dict(by=None), dict(rank=None), dict(parent=None), dict(order=None), dict(first=a, parent=None)):
        bad(INVALID, "hpcla_rcm_narrow", good, **kw)
    bad(UNSUPPORTED, "hpcla_rcm_narrow", good, nrows=big)
    good = dict(g_rowptr=a, g_cols=a, nrows=4, order=a, lo=1, hi=2, longest=3, parent=a, cand=a, count=a, stream=None)
    for kw in (dict(nrows=-1), dict(lo=3), dict(lo=-1), dict(hi=5), dict(longest=-1), dict(count=None), dict(g_rowptr=None), dict(g_cols=None),
               dict(order=None), dict(parent=None), dict(cand=None)):
        bad(INVALID, "hpcla_rcm_expand", good, **kw)
    bad(UNSUPPORTED, "hpcla_rcm_expand", good, nrows=big)
    good = dict(cand=a, ncand=2, nrows=4, parent=a, rank=a, keys=a, stream=None)
    for kw in (dict(nrows=-1), dict(ncand=-1), dict(ncand=5), dict(cand=None), dict(parent=None), dict(rank=None), dict(keys=None)):
        bad(INVALID, "hpcla_rcm_keys", good, **kw)
    bad(UNSUPPORTED, "hpcla_rcm_keys", good, nrows=big)
    good = dict(keys=a, ncand=2, nrows=4, by=a, cnt=1, order=a, stream=None)
    for kw in (dict(nrows=-1), dict(ncand=-1), dict(ncand=5), dict(cnt=-1), dict(cnt=3), dict(keys=None), dict(by=None), dict(order=None)):
        bad(INVALID, "hpcla_rcm_number", good, **kw)
    bad(UNSUPPORTED, "hpcla_rcm_number", good, nrows=big)
    good = dict(order=a, nrows=4, row_start=0, p=a, inv=a, stream=None)
    for kw in (dict(nrows=-1), dict(order=None), dict(p=None), dict(inv=None)):
        bad(INVALID, "hpcla_rcm_finish", good, **kw)
    bad(UNSUPPORTED, "hpcla_rcm_finish", good, nrows=big)
    good = dict(g_rowptr=a, g_cols=a, nrows=4, inv=None, out=a, stream=None)
    for kw in (dict(nrows=-1), dict(out=None), dict(g_rowptr=None)):
        bad(INVALID, "hpcla_rcm_graph_bandwidth", good, **kw)
    bad(UNSUPPORTED, "hpcla_rcm_graph_bandwidth", good, nrows=big)
    assert np.all(_host(a) == 0)                                     # nothing wrote into what stood for the arrays


def test_no_rows_need_no_arrays(hp):
    """Status 0 with NULL arrays at size 0; the one-workgroup kernel reports an empty walk as done."""
    out = _full(8, BEHIND, I64)
    _call(hp, "hpcla_rcm_degrees", None, None, 0, 1, None, None)
    _call(hp, "hpcla_rcm_init", None, None, 0, None, None, None, out, None)
    assert _host(out).tolist() == [0] + [BEHIND] * 7
    out.fill_(BEHIND)
    _call(hp, "hpcla_rcm_expand", None, None, 0, None, 0, 0, 0, None, None, out, None)
    assert _host(out).tolist() == [0] + [BEHIND] * 7
    _call(hp, "hpcla_rcm_keys", None, 0, 0, None, None, None, None)
    _call(hp, "hpcla_rcm_number", None, 0, 0, None, 0, None, None)
    _call(hp, "hpcla_rcm_finish", None, 0, 0, None, None, None)
    out.fill_(BEHIND)
    _call(hp, "hpcla_rcm_narrow", None, None, None, None, 0, 0, 0, 0, None, None, None, out, None)
    assert _host(out).tolist() == [0, 0, 0, rc.DONE, 0, 0, BEHIND, BEHIND]
