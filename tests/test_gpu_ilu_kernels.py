"""GPU tests of the eleven C entries of csrc/ilu.hip ON THEIR OWN, through the C ABI (``hp._capi``), on inputs ``hp.ilu0`` never
builds: one block of a row partition at a time with its ghost columns, both index widths, ``index_base`` 0 and 1, rows in any
stored order, rows past several scan blocks, faults that the caller ignores, and every lane count of the triangular sweep.

1. The chain count / fill / gather / init / sweep x 3 / pivots on every block of ``ic.kernel_cases`` (every factor case, the
   65 x 63 one included, in 1, 2, 3 and 8 blocks; ``arrow`` and ``comb`` whole), after every launch.  Every block runs with Int32
   indices and base 0; the 3- and 8-block cuts of ``ic.KERNEL_FORMS_ON`` run the other three forms too, which give the same bits.
2. count / fill alone: the row counts of ``ic.ROW_EDGES`` (up to the first size that needs the carry of the scan's second
   phase), no rows at all, shuffled rows, duplicated columns, the fill's error word on ``ic.three_faults``.
3. The per-entry kernels at ``ic.NNZ_EDGES``; faults and special values through init / sweep / pivots with the word ignored; the
   pivots alone on hand-filled diagonals.
4. ``hpcla_ilu_trisweep_f64`` alone on ``ic.ragged`` at ``ic.RAGGED_SIZES`` x lanes x upper x (in, dinv given or NULL), on views
   8 bytes into their buffers, on ``arrow`` and ``banded16``; ``hpcla_ilu_apply_f64`` at every ``solve_sweeps``, with out == r.
5. ``update`` of an ``hp.ilu0`` object with new values, a failing one among them, and healed again.

Expected values: tests/_ilu_cases.py restates each kernel one rounded operation at a time in the order csrc/ilu.hip states, and
the library is built with -ffp-contract=off, so every comparison here is exact: integers, or the bits of the doubles (where a
fault is put in on purpose, NaN against NaN without its payload).  The two margins that appear, ``ic.ILU_RTOL`` and the
application's 1e-12, are those of tests/test_gpu_ilu0.py; tests/_ilu_cases.py has their bases.  No margin is introduced here.

Which slip which test catches (argued from csrc/ilu.hip, not from runs of broken kernels):
  a dropped ``- base`` in count or fill        the base-1 forms of test_chain_on_every_block, of the row-count edges, of the
                                               shuffled and the duplicated rows: other rows are read, or ghosts become owned
  ``c <= n_own`` for ``c < n_own``             the first ghost id is n_own in every block with ghosts: one entry too many
  the tie rule ``e2 < e`` removed              test_duplicated_columns: two entries get one rank, a position stays BEHIND
  b_rowptr[nrows] not written when the last    nrows = 1025, 2049 and 262 145 of test_structure_at_the_row_count_edges, where
  row opens a scan block                       nrows - 1 is a multiple of SCAN_B: b_rowptr[nrows] and info[0] stay as given
  the scan carry dropped                       nrows = 262 145: the offset of block 256
  ``kr > m`` for ``kr >= m``                   every chain with an entry below the diagonal: l_ij u_jj joins the sum
  ``++rp`` and ``++cq`` swapped                every merge that skips: the stencils, ``asymmetric``, ``comb`` (an entry with five
                                               skips of each kind, tests/test_ilu_cases.py counts them); ``arrow`` never skips
  f_new[dj] for f_old[dj]                      the values after each sweep (another launch's or no value is read: f_new starts
                                               at BEHIND_F)
  a fused multiply-subtract, another order     the bit comparison after every launch, which ILU_RTOL cannot see; ``arrow``'s corner
                                               sums 299 products across a binade, so its bits depend on the order
  atomicMax for atomicMin                      the fill's word on three faults, test_pivots_alone (failing rows in three
                                               workgroups, the word coming in above, below and at the first of them)
  the Inf test missing from the pivots         test_pivots_alone's +Inf and -Inf rows, ``inf_diagonal`` of the faults
  ``lo = dp`` in the upper sweep               every upper = 1 call of test_trisweep_alone: the diagonal joins the sum
  a lane group split across the ``live`` edge  rows * lanes on, just below and just above a multiple of 256, 1 row, 1023 rows
  spare and out swapped for one parity         test_apply_at_every_sweep_count: both parities, out's bits and the words behind
  the error word not reset in ``update``       test_update_with_new_values_a_failure_and_a_heal: the heal after the failure
"""
import time

import numpy as np
import pytest

from tests import _amg_cases as ac
from tests import _ilu_cases as ic
from tests import _pcg_cases as pc
from tests.test_gpu_precond_kernels import FORM_IDS, FORMS, _call, _dev, _full, _host, _same, _torch

pytestmark = pytest.mark.gpu

F64, I64, I32 = np.float64, np.int64, np.int32
BEHIND = -7                                                      # the word behind every integer output
BEHIND_F = -7.25                                                 # and behind every double output
RAN = {}                                                         # case name -> what its chains covered


@pytest.fixture(scope="module")
def matrices(orc):
    return ic.kernel_cases(orc)


def _same_but_nan(got, want, what):
    """NaN where the restatement has NaN (whatever the payload), the restatement's bits everywhere else."""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions", np.flatnonzero(np.isnan(got) != np.isnan(want))[:5])
    keep = ~np.isnan(want)
    _same(got[keep], want[keep], what)


# ---- the chain of entries on one block ----------------------------------------------------------------------------------------------
def _structure(hp, split, n, form, tag):
    """count, fill and gather on rows in split form (0-based host arrays; the form's base and type are put on here).  Every
    output has one word more than it needs, and ``work`` exactly the words ``hpcla_ilu_work_bytes`` asks for and one behind."""
    sfx, Ti, base = form
    rowptr, colval, vals = split
    d_rowptr, d_colval, d_vals = _dev(np.asarray(rowptr) + base, Ti), _dev(np.asarray(colval) + base, Ti), _dev(vals, F64)
    words = hp._capi.load().hpcla_ilu_work_bytes(n) // 8
    work = _full(words + 1, BEHIND, I64)
    b_rowptr, info = _full(n + 2, BEHIND, I32), _full(3, BEHIND, I64)
    _call(hp, f"hpcla_ilu_count_f64_{sfx}", d_rowptr, d_colval, n, n, base, b_rowptr, info, work, None)
    assert int(_host(work)[words]) == BEHIND, (tag, "the word behind work")
    bp = _host(b_rowptr)
    nnz = int(bp[n])
    assert bp[n + 1] == BEHIND and _host(info).tolist() == [nnz, -1, BEHIND], (tag, "count", _host(info).tolist())
    b_cols, b_rows, b_diag = _full(nnz + 1, BEHIND, I32), _full(nnz + 1, BEHIND, I32), _full(n + 1, BEHIND, I32)
    b_map, a_vals = _full(nnz + 1, BEHIND, I64), _full(nnz + 1, BEHIND_F, F64)
    _call(hp, f"hpcla_ilu_fill_f64_{sfx}", d_rowptr, d_colval, d_vals, n, n, base, b_rowptr, b_cols, b_rows, b_diag, b_map, info, None)
    _call(hp, "hpcla_ilu_gather_f64", d_vals, b_map, nnz, a_vals, None)
    got = dict(n=n, nnz=nnz, bp=bp[:n + 1], bc=_host(b_cols), brows=_host(b_rows), bdiag=_host(b_diag), bmap=_host(b_map),
               a_vals=_host(a_vals), info=_host(info).tolist())
    assert got["bc"][nnz] == got["brows"][nnz] == got["bmap"][nnz] == got["bdiag"][n] == BEHIND, (tag, "a word behind the block")
    assert got["a_vals"][nnz] == BEHIND_F and got["info"][0] == nnz and got["info"][2] == BEHIND, (tag, got["info"])
    for what in ("bc", "brows", "bmap", "a_vals"):
        got[what] = got[what][:nnz]
    got["bdiag"], got["word"] = got["bdiag"][:n], got["info"][1]
    got["dev"] = dict(b_rowptr=b_rowptr, b_cols=b_cols, b_rows=b_rows, b_diag=b_diag, a_vals=a_vals, info=info)
    return got


def _check_structure(got, want, tag, values=_same):
    for what in ("bp", "bc", "brows", "bdiag", "bmap"):
        _same(got[what].astype(I64), want[what], (tag, what))
    values(got["a_vals"], want["a_vals"], (tag, "a_vals"))
    assert got["word"] == want["word"], (tag, "the fill's word", got["word"], want["word"])


def _factor(hp, got, want, tag, values=_same):
    """init, three sweeps between two buffers and the pivots on the block ``_structure`` left on the device; after every launch
    the values are ``want``'s, the buffer read is unchanged and the word behind the buffer written is where it was."""
    dev, n, nnz = got["dev"], got["n"], got["nnz"]
    c_ptr, c_pos = _dev(want["c_ptr"], I32), _dev(want["c_pos"], I32)       # the caller's stable sort (csrc/ilu.hip)
    index = (dev["b_cols"], dev["b_rows"], dev["b_diag"])
    f, g = _full(nnz + 1, BEHIND_F, F64), _full(nnz + 1, BEHIND_F, F64)
    _call(hp, "hpcla_ilu_init_f64", *index, dev["a_vals"], nnz, f, None)
    out = [_host(f)]
    values(out[0][:nnz], want["f"][0], (tag, "init"))
    assert out[0][nnz] == BEHIND_F, (tag, "the word behind f")
    for t in range(1, len(want["f"])):
        g.fill_(BEHIND_F)
        _call(hp, "hpcla_ilu_sweep_f64", dev["b_rowptr"], *index, c_ptr, c_pos, dev["a_vals"], f, g, nnz, None)
        out.append(_host(g))
        values(out[t][:nnz], want["f"][t], (tag, f"sweep {t}"))
        assert out[t][nnz] == BEHIND_F, (tag, f"the word behind f_new, sweep {t}")
        assert np.array_equal(pc.bits(_host(f)), pc.bits(out[t - 1])), (tag, f"f_old changed in sweep {t}")
        f, g = g, f
    dinv = _full(n + 1, BEHIND_F, F64)
    _call(hp, "hpcla_ilu_pivots_f64", dev["b_diag"], f, n, dinv, dev["info"], None)
    want_dinv, want_word = ic.pivots(want["bdiag"], want["f"][-1], want["word"])
    got_dinv, info = _host(dinv), _host(dev["info"]).tolist()
    _same_but_nan(got_dinv[:n], want_dinv, (tag, "dinv"))
    assert got_dinv[n] == BEHIND_F and info == [nnz, want_word, BEHIND], (tag, "pivots", info, want_word)
    _same(_host(dev["a_vals"])[:nnz], got["a_vals"], (tag, "a_vals after the chain"))
    return dict(f=[o[:nnz] for o in out], dinv=got_dinv[:n], word=info[1])


def _chain(hp, want, form, tag, values=_same):
    got = _structure(hp, want["split"], want["n"], form, tag)
    _check_structure(got, want, tag, values)
    got.update(_factor(hp, got, want, tag, values))
    return got


def _agree(got, first, tag):
    """Two index forms of one block: the same integers and the same bits (NaN payloads included: the same instructions ran)."""
    for what in ("bp", "bc", "brows", "bdiag", "bmap", "a_vals", "dinv"):
        _same(got[what], first[what], (tag, what, "against the first form"))
    for t, (a, b) in enumerate(zip(got["f"], first["f"])):
        _same(a, b, (tag, f"f after launch {t}", "against the first form"))
    assert got["word"] == first["word"], tag


# ---- 1. every block of every case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["convdiff16x16", "convdiff24x20", "convdiff33x31", "convdiff%dx%d" % pc.LARGE_SIZE] +
                         [f"banded{w}" for w in ic.BANDED_W] + ["asymmetric", "diagonal", "one", "arrow", "comb"])
def test_chain_on_every_block(hp, matrices, name):
    t0 = time.perf_counter()
    matrix = matrices[name]
    stats = dict(chains=0, runs=0, rows=0, ghosts=0, longest=0)
    for k, j, part in ic.block_inputs(name, matrix):
        want = ic.block_reference(matrix, part, j)
        forms = FORMS if name in ic.KERNEL_FORMS_ON and k in ic.KERNEL_FORMS_BLOCKS else FORMS[:1]
        first = None
        for form in forms:
            tag = (name, k, j, form[0], form[2])
            got = _chain(hp, want, form, tag)
            assert got["word"] == ic.NO_FAILURE, tag
            first = first or got
            _agree(got, first, tag)
            stats["runs"] += 1
        stats["chains"] += 1
        stats["rows"] = max(stats["rows"], want["n"])
        stats["ghosts"] += want["ghosts"]
        stats["longest"] = max(stats["longest"], int(want["products"][3][:, 0].max()))
    RAN[name] = stats
    print(f"{name}: {stats['chains']} blocks, {stats['runs']} chains run, largest block {stats['rows']} rows, {stats['ghosts']} ghost "
          f"columns, longest merged sum {stats['longest']} products, {time.perf_counter() - t0:.2f} s")
    assert stats["chains"] >= 1
    if name == "convdiff%dx%d" % pc.LARGE_SIZE:
        assert stats["rows"] == 4095 and stats["runs"] == 14 + 3 * 11
    if name == "arrow":
        assert stats["longest"] == ic.ARROW_N - 1


def test_the_chains_that_ran(matrices):
    """The totals of the parametrised test above, where it ran in this session."""
    if set(RAN) != set(matrices):
        return
    chains, runs = sum(s["chains"] for s in RAN.values()), sum(s["runs"] for s in RAN.values())
    print(f"{chains} (case, blocks, block) inputs, {runs} (case, blocks, block, form) chains, longest merged sum "
          f"{max(s['longest'] for s in RAN.values())} products")
    assert chains >= 150 and runs == chains + 3 * 11 * len(ic.KERNEL_FORMS_ON)


# ---- 2. count and fill alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ic.ROW_EDGES)
def test_structure_at_the_row_count_edges(hp, n):
    rowptr, colval, vals = ic.generated_rows(n)
    want = dict(zip(("bp", "bc", "brows", "bdiag", "bmap", "a_vals", "word"), ic.block_of_split(rowptr, colval, vals, n)))
    for form in (FORMS[0], FORMS[3]):
        got = _structure(hp, (rowptr, colval, vals), n, form, (n, form[0], form[2]))
        _check_structure(got, want, (n, form[0], form[2]))
        assert got["nnz"] == len(want["bc"]) and got["word"] == ic.NO_FAILURE


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_no_rows(hp, form):
    sfx, _, base = form
    b_rowptr, info, work = _full(2, BEHIND, I32), _full(3, BEHIND, I64), _full(3, BEHIND, I64)
    _call(hp, f"hpcla_ilu_count_f64_{sfx}", None, None, 0, 0, base, b_rowptr, info, work, None)
    assert _host(b_rowptr).tolist() == [0, BEHIND] and _host(info).tolist() == [0, -1, BEHIND]
    _call(hp, f"hpcla_ilu_fill_f64_{sfx}", None, None, None, 0, 0, base, None, None, None, None, None, info, None)
    _call(hp, "hpcla_ilu_gather_f64", None, None, 0, None, None)
    _call(hp, "hpcla_ilu_init_f64", None, None, None, None, 0, None, None)
    _call(hp, "hpcla_ilu_pivots_f64", None, None, 0, None, info, None)
    _call(hp, "hpcla_ilu_trisweep_f64", None, None, None, None, None, None, None, None, 0, 0, 1, None)
    assert _host(info).tolist() == [0, -1, BEHIND] and _host(work).tolist() == [BEHIND] * 3


@pytest.mark.parametrize("name", ic.SHUFFLED_ON)
def test_rows_in_any_stored_order(hp, matrices, name):
    """Every row's entries permuted, so ghosts stand anywhere among the owned ones: the block of the sorted input, ``bmap`` at
    the shuffled positions."""
    matrix = matrices[name]
    part = ic.equal_blocks(len(matrix[0]) - 1, 3)
    for j in range(3):
        want = ic.block_reference(matrix, part, j, sweeps=0)
        rowptr, split, vals = want["split"]
        cols2, vals2, perm = ic.shuffled_rows(rowptr, split, vals, np.random.default_rng(5 + j))
        shuffled = dict(zip(("bp", "bc", "brows", "bdiag", "bmap", "a_vals", "word"), ic.block_of_split(rowptr, cols2, vals2, want["n"])))
        for form in FORMS:
            tag = (name, j, form[0], form[2])
            got = _structure(hp, (rowptr, cols2, vals2), want["n"], form, tag)
            _check_structure(got, shuffled, tag)
            for what in ("bp", "bc", "brows", "bdiag"):
                _same(got[what].astype(I64), want[what], (tag, what, "against the sorted input"))
            _same(got["a_vals"], want["a_vals"], (tag, "a_vals against the sorted input"))
            _same(perm[got["bmap"]], want["bmap"], (tag, "bmap through the permutation"))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_duplicated_columns(hp, form):
    """Structure only: ties in stored order, the diagonal at its last stored duplicate (whose value the word is about)."""
    rowptr, split, vals, n_own = ic.duplicated_block()
    want = dict(zip(("bp", "bc", "brows", "bdiag", "bmap", "a_vals", "word"), ic.block_of_split(rowptr, split, vals, n_own)))
    got = _structure(hp, (rowptr, split, vals), n_own, form, ("duplicates", form))
    _check_structure(got, want, ("duplicates", form))
    assert got["bdiag"].tolist() == [1, 5, 7, 10] and got["word"] == (1 << 2) | ic.BAD_DIAG


def test_the_fills_word_names_the_smallest_failing_row(hp):
    for heal in range(4):
        rowptr, cols, vals = ic.three_faults(heal)
        want = ic.block_of_split(rowptr, cols, vals, 600)
        for form in (FORMS[0], FORMS[3]):
            got = _structure(hp, (rowptr, cols, vals), 600, form, ("three faults", heal, form))
            assert got["word"] == want[6] == (-1 if heal == 3 else (ic.FAULT_ROWS[heal] << 2) | (ic.NO_DIAG if heal == 1 else ic.BAD_DIAG))
            assert (got["bdiag"][300] == -1) == (heal < 2)
            _same(got["bdiag"].astype(I64), want[3], ("three faults", heal, "bdiag"))
            _same_but_nan(got["a_vals"], want[5], ("three faults", heal, "a_vals"))


# ---- 3. the per-entry kernels, faults, pivots -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nnz", ic.NNZ_EDGES)
def test_per_entry_kernels_at_the_workgroup_edges(hp, nnz):
    matrix = ic.nnz_edge(nnz)
    want = ic.block_reference(matrix, [0, len(matrix[0]) - 1], 0)
    assert len(want["bc"]) == nnz
    got = _chain(hp, want, FORMS[0], ("nnz", nnz))
    assert got["nnz"] == nnz and got["word"] == ic.NO_FAILURE


def test_faults_spoil_the_rows_from_their_own_on_only(hp):
    """The kernels called with the error word ignored.  Rows above the fault keep the clean matrix's bits after three sweeps;
    from the fault's row on NaN stands where the restatement has NaN and every other entry has its bits, signed zeros included."""
    r, n = ic.FAULT_ROW, ic.BANDED_N
    clean = _chain(hp, ic.block_reference(ic.fault_case(None), [0, n], 0), FORMS[0], ("clean",))
    head = int(clean["bp"][r])
    for kind in ic.FAULT_KINDS:
        want = ic.block_reference(ic.fault_case(kind), [0, n], 0)
        got = _chain(hp, want, FORMS[0], (kind,), values=_same_but_nan)
        assert int(got["bp"][r]) == head, kind
        for t in range(4):
            _same(got["f"][t][:head], clean["f"][t][:head], (kind, f"rows above the fault after launch {t}"))
        _same(got["dinv"][:r], clean["dinv"][:r], (kind, "dinv above the fault"))
        structural = {"nan_diagonal": ic.BAD_DIAG, "no_diagonal": ic.NO_DIAG, "zero_diagonal": ic.BAD_DIAG}
        if kind in structural:
            assert got["word"] == (r << 2) | structural[kind], (kind, got["word"])
        elif kind == "negative_zero_off":
            assert got["word"] == ic.NO_FAILURE and np.isfinite(got["f"][3]).all()
            zero = int(np.flatnonzero((want["brows"] == r) & (want["bc"] == r - 2))[0])
            assert got["f"][0][zero] == 0.0 and np.signbit(got["f"][0][zero])
        else:
            assert got["word"] >> 2 >= r and got["word"] & 3 == ic.BAD_PIVOT, (kind, got["word"])


@pytest.mark.parametrize("n", ic.PIVOT_SIZES)
def test_pivots_alone(hp, n):
    bdiag, f = ic.pivot_case(n)
    inputs = [(bdiag, f)]
    if n == 1:
        inputs = [(bdiag, np.array([v])) for v in ic.PIVOT_SPECIALS + [3.0]] + [(np.array([-1]), f)]
    for bd, fv in inputs:
        first = ic.pivots(bd, fv)[1]
        words = [ic.NO_FAILURE, (0 << 2) | ic.NO_DIAG, ((n + 5) << 2) | ic.BAD_DIAG]
        if first != ic.NO_FAILURE:
            words += [((first >> 2) << 2) | ic.NO_DIAG, ((first >> 2) << 2) | ic.BAD_DIAG]
            if first >> 2 > 0:
                words.append(((first >> 2) - 1) << 2 | ic.BAD_PIVOT)
        d_diag, d_f = _dev(bd, I32), _dev(fv, F64)
        for word_in in words:
            want_dinv, want_word = ic.pivots(bd, fv, word_in)
            dinv, info = _full(n + 1, BEHIND_F, F64), _dev([BEHIND, word_in, BEHIND], I64)
            _call(hp, "hpcla_ilu_pivots_f64", d_diag, d_f, n, dinv, info, None)
            got = _host(dinv)
            _same_but_nan(got[:n], want_dinv, (n, word_in, "dinv"))
            assert got[n] == BEHIND_F and _host(info).tolist() == [BEHIND, want_word, BEHIND], (n, fv[:1], word_in, _host(info).tolist())
        _same(_host(d_f)[:len(fv)], fv, (n, "f"))


# ---- 4. the triangular sweep and the application ----------------------------------------------------------------------------------------
def _trisweep_inputs(bp, bc, bdiag, f, seed):
    n = len(bp) - 1
    rng = np.random.default_rng(seed)
    return dict(n=n, bp=bp, bc=bc, bdiag=bdiag, f=f, rhs=rng.uniform(-1, 1, n), inp=rng.uniform(-1, 1, n), dinv=1.0 / f[bdiag],
                d_bp=_dev(bp, I32), d_bc=_dev(bc, I32), d_bdiag=_dev(bdiag, I32), d_f=_dev(f, F64))


def _inside(values, shift):
    """(buffer, the operand ``shift`` doubles into it, with one word behind it)."""
    torch = _torch()
    n = len(values)
    buf = torch.full((n + shift + 2,), BEHIND_F, dtype=torch.float64, device="cuda")
    buf[shift:shift + n].copy_(torch.from_numpy(np.array(values, dtype=F64)))
    return buf, buf[shift:shift + n]


def _trisweep_check(hp, c, lanes_list, tag, shift=0):
    n = c["n"]
    (rb, rhs), (ib, inp), (db, dinv) = (_inside(c[what], shift) for what in ("rhs", "inp", "dinv"))
    snaps = [b.clone() for b in (rb, ib, db, c["d_f"])]
    assert all(v.data_ptr() % 16 == 8 * (shift & 1) for v in (rhs, inp))
    for lanes in lanes_list:
        for upper in (0, 1):
            for with_in in (True, False):
                for with_dinv in (True, False):
                    ob, out = _inside(np.full(n, BEHIND_F), shift)
                    _call(hp, "hpcla_ilu_trisweep_f64", c["d_bp"], c["d_bc"], c["d_bdiag"], c["d_f"], rhs, inp if with_in else None,
                          dinv if with_dinv else None, out, n, upper, lanes, None)
                    want = ic.trisweep(c["bp"], c["bc"], c["bdiag"], c["f"], c["rhs"], c["inp"] if with_in else None,
                                       c["dinv"] if with_dinv else None, upper, lanes)
                    whole = _host(ob)
                    _same(whole[shift:shift + n], want, (tag, lanes, upper, with_in, with_dinv, "out"))
                    assert np.all(whole[:shift] == BEHIND_F) and np.all(whole[shift + n:] == BEHIND_F), (tag, lanes, upper, "around out")
    for b, snap in zip((rb, ib, db, c["d_f"]), snaps):
        assert np.array_equal(pc.bits(_host(b)), pc.bits(_host(snap))), (tag, "rhs, in, dinv or f changed")


@pytest.mark.parametrize("n", ic.RAGGED_SIZES)
def test_trisweep_alone(hp, n):
    bp, bcols, brows, bdiag, bmap, f, word = ic.block_of_split(*ic.ragged(n), n)
    c = _trisweep_inputs(bp, bcols, bdiag, f, n)
    _trisweep_check(hp, c, ic.LANES, ("ragged", n))
    if n == 257:
        _trisweep_check(hp, c, ic.LANES, ("ragged", n, "8 bytes in"), shift=1)


@pytest.mark.parametrize("name", ["arrow", "banded16"])
def test_trisweep_on_a_long_row_and_on_bands(hp, matrices, name):
    matrix = matrices[name]
    want = ic.block_reference(matrix, [0, len(matrix[0]) - 1], 0)
    c = _trisweep_inputs(want["bp"], want["bc"], want["bdiag"], want["f"][3], 11)
    _trisweep_check(hp, c, (1, 8), (name,))


@pytest.mark.parametrize("name", ["ragged257", "arrow"])
def test_apply_at_every_sweep_count(hp, matrices, name):
    """out against the chain of launches restated, r untouched; with out == r the bits of the two-buffer call."""
    if name == "arrow":
        want = ic.block_reference(matrices[name], [0, ic.ARROW_N], 0)
        bp, bcols, bdiag, f = want["bp"], want["bc"], want["bdiag"], want["f"][3]
    else:
        bp, bcols, _, bdiag, _, f, _ = ic.block_of_split(*ic.ragged(257), 257)
    c = _trisweep_inputs(bp, bcols, bdiag, f, 23)
    n = c["n"]
    r, dinv = _dev(c["rhs"], F64), _dev(c["dinv"], F64)
    t0, t1 = _full(n + 1, BEHIND_F, F64), _full(n + 1, BEHIND_F, F64)
    index = (c["d_bp"], c["d_bc"], c["d_bdiag"], c["d_f"], dinv)
    for lanes in (1, 8):
        for s in range(1, 17):
            want_z = ic.apply_chain(bp, bcols, bdiag, f, c["dinv"], c["rhs"], s, lanes)
            out = _full(n + 1, BEHIND_F, F64)
            _call(hp, "hpcla_ilu_apply_f64", *index, r, t0, t1, out, n, s, lanes, None)
            got = _host(out)
            _same(got[:n], want_z, (name, lanes, s, "out"))
            assert got[n] == BEHIND_F and _host(t0)[n] == BEHIND_F and _host(t1)[n] == BEHIND_F, (name, lanes, s, "a word behind")
            _same(_host(r), c["rhs"], (name, lanes, s, "r"))
            both = _full(n + 1, BEHIND_F, F64)
            both[:n].copy_(r)
            _call(hp, "hpcla_ilu_apply_f64", *index, both, t0, t1, both, n, s, lanes, None)
            _same(_host(both), got, (name, lanes, s, "out == r"))
    want_z = ic.apply(bp, bcols, f, c["rhs"], 3)
    z = ic.apply_chain(bp, bcols, bdiag, f, c["dinv"], c["rhs"], 3, 1)
    assert np.allclose(z, want_z, rtol=1e-12, atol=1e-12 * np.abs(want_z).max())


# ---- 5. new values on an old structure --------------------------------------------------------------------------------------------------
def test_update_with_new_values_a_failure_and_a_heal(hp, gpu_backend_i32):
    rowptr, colidx, vals = ic.banded(8)
    n, r = ic.BANDED_N, ic.FAULT_ROW
    mk = lambda v: hp.HPCSparseMatrix_local(rowptr, colidx, v, n, gpu_backend_i32)
    M = hp.ilu0(mk(vals))
    first = pc.bits(M.factors()[2]).copy()
    scale = np.random.default_rng(8).uniform(0.5, 2.0, n)
    scaled = vals * np.repeat(scale, np.diff(rowptr))
    f = M.update(mk(scaled)).factors()[2]
    bp, bcols, bv = ic.block_csr(rowptr, colidx, scaled)
    want = ic.sweep_factors(bp, bcols, bv, 3)
    dev = float(np.max(np.abs(f - want) / np.abs(want)))
    print(f"update with rows scaled: largest relative deviation {dev:.2e}, bit for bit: {np.array_equal(pc.bits(f), pc.bits(want))}")
    assert dev <= ic.ILU_RTOL and not np.array_equal(pc.bits(f), first)
    assert np.array_equal(pc.bits(hp.ilu0(mk(scaled)).factors()[2]), pc.bits(f))
    broken = scaled.copy()
    broken[int(rowptr[r] + np.flatnonzero(colidx[rowptr[r]:rowptr[r + 1]] == r)[0])] = 0.0
    with pytest.raises(ValueError, match=rf"^ilu0: the diagonal of row {r} is zero or NaN$"):
        M.update(mk(broken))
    with pytest.raises(ValueError, match=rf"^ilu0: the diagonal of row {r} is zero or NaN$"):
        hp.ilu0(mk(broken))
    assert np.array_equal(pc.bits(M.update(mk(vals)).factors()[2]), first)
    assert np.array_equal(pc.bits(M.update(mk(scaled)).factors()[2]), pc.bits(f))
    hp.clear_plan_cache()
