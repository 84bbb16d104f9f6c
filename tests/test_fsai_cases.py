"""CPU side of the factorised sparse approximate inverse preconditioner: the public names, the C ABI tables, the argument rules
that need no device, and the numpy restatements of tests/_fsai_cases.py against each other and on the shared cases."""
import os
import re
import sys

import numpy as np
import pytest

from tests import _fsai_cases as fc
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_fsai_work_bytes", "hpcla_fsai_count_f64_i32", "hpcla_fsai_count_f64_i64", "hpcla_fsai_factor_f64_i32",
               "hpcla_fsai_factor_f64_i64", "hpcla_pcg_fsai_iterations_f64_i32", "hpcla_pcg_fsai_iterations_f64_i64"]


@pytest.fixture(scope="module")
def cases(orc):
    """Every SPD case with both restatements of G, computed once."""
    out = {}
    for name, (rowptr, colidx, vals, b, pat) in fc.spd_cases(orc).items():
        out[name] = dict(rowptr=rowptr, colidx=colidx, vals=vals, b=b, pattern=pat,
                         G=fc.fsai_cholesky(rowptr, colidx, vals, pattern=pat), G2=fc.fsai_solve(rowptr, colidx, vals, pattern=pat))
    return out


def test_public_names_exist(hp):
    assert callable(hp.fsai) and hp.FSAI
    assert hp.fsai.__module__.endswith("fsai")
    assert "FSAI" in hp.cg.__doc__ and "32" in hp.fsai.__doc__


def test_header_declares_the_new_entries_and_ctypes_binds_them(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in hp._capi.EXPORTED_SYMBOLS, name
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hpcla_rocm.h"
        assert m.group(1).count(",") + 1 == len(hp._capi._SIGNATURES[name]), name
    sig = hp._capi._SIGNATURES
    # the plan / CSR block three times (A, G, Gt) where hpcla_pcg_iterations_* has it once, two more vectors (u, z), no dinv
    for sfx, block in (("i32", 13), ("i64", 11)):
        assert len(sig[f"hpcla_pcg_fsai_iterations_f64_{sfx}"]) == len(sig[f"hpcla_pcg_iterations_f64_{sfx}"]) + 2 * block + 2 - 1
    lib = hp._capi.load()
    assert lib.hpcla_fsai_work_bytes(0) == 16 and lib.hpcla_fsai_work_bytes(1024) == 16 and lib.hpcla_fsai_work_bytes(1025) == 24


def test_c_entries_refuse_bad_arguments_without_a_gpu(hp):
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    one = 8                                                              # any non-null address: refused before it is looked at
    assert lib.hpcla_fsai_count_f64_i32(None, None, None, None, -1, -1, 0, one, one, one, None) == INVALID       # negative size
    assert lib.hpcla_fsai_count_f64_i64(None, None, None, None, 4, 5, 0, one, one, one, None) == INVALID         # n_own != nrows
    assert lib.hpcla_fsai_count_f64_i32(None, None, None, None, 4, 4, 2, one, one, one, None) == INVALID         # index_base
    assert lib.hpcla_fsai_count_f64_i32(None, None, None, None, 4, 4, 0, None, one, one, None) == INVALID        # null rowptr out
    for max_m in (0, 33):
        assert lib.hpcla_fsai_factor_f64_i32(*([None] * 5), 4, 4, 0, 0, max_m, one, one, one, one, None) == INVALID
    assert lib.hpcla_fsai_factor_f64_i64(*([None] * 5), 4, 4, 0, 0, 8, one, one, one, one, None) == INVALID      # null CSR arrays
    assert lib.hpcla_fsai_factor_f64_i64(*([None] * 5), 0, 0, 0, 0, 8, None, None, None, one, None) == 0         # no rows: nothing to do
    blk32, blk64 = [None] * 6 + [4, 0, 0, None, 0, None, 0], [None] * 4 + [4, 0, 0, None, 0, None, 0]
    tail = [None] * 10
    assert lib.hpcla_pcg_fsai_iterations_f64_i32(None, *blk32, *blk32, *blk32, *tail, 1, -1, None) == INVALID
    assert lib.hpcla_pcg_fsai_iterations_f64_i64(None, *blk64, *blk64, *blk64, *tail, 0, 1, None) == INVALID


def test_argument_rules_that_need_no_device(hp):
    mod = sys.modules[hp.fsai.__module__]
    part = np.array([0, 5, 10])
    mod.check_arguments(np.float64, (10, 10), part, part)
    mod.check_arguments(np.float64, (10, 10), part, part, ((10, 10), part, part))
    with pytest.raises(ValueError, match="square"):
        mod.check_arguments(np.float64, (10, 12), part, np.array([0, 6, 12]))
    with pytest.raises(TypeError, match="Float64"):
        mod.check_arguments(np.float32, (10, 10), part, part)
    with pytest.raises(ValueError, match="partitioned alike"):
        mod.check_arguments(np.float64, (10, 10), part, np.array([0, 4, 10]))
    with pytest.raises(ValueError, match="pattern"):
        mod.check_arguments(np.float64, (10, 10), part, part, ((10, 10), np.array([0, 4, 10]), part))
    with pytest.raises(ValueError, match="pattern"):
        mod.check_arguments(np.float64, (10, 10), part, part, ((12, 12), part, part))
    assert mod.error_message(3, 17) == "fsai: A is not positive definite on the pattern of row 17"
    assert mod.error_message(1, 40).startswith("fsai: a pattern row has more than 32 owned entries")
    assert mod.error_message(2, 4) == "fsai: row 4 stores no diagonal"


def test_the_two_restatements_agree(cases):
    worst = 0.0
    for name, c in cases.items():
        (p1, c1, v1), (p2, c2, v2) = c["G"], c["G2"]
        assert np.array_equal(p1, p2) and np.array_equal(c1, c2), name
        dev = float(np.max(np.abs(v1 - v2) / np.abs(v1)))
        print(f"{name}: largest relative difference of an entry {dev:.2e}, largest row {np.diff(p1).max()}")
        worst = max(worst, dev)
    print(f"worst {worst:.3e}; FSAI_RTOL {fc.FSAI_RTOL:.1e}")
    assert pc.LARGE_MARGIN_FACTOR * worst <= fc.FSAI_RTOL


def test_structure_of_G(cases):
    for w in fc.BANDED_W:
        gp = cases[f"banded{w}"]["G"][0]
        assert np.array_equal(np.diff(gp), np.minimum(np.arange(fc.BANDED_N), w) + 1), w
    classes = {4 if m <= 4 else 8 if m <= 8 else 16 if m <= 16 else 32 for w in fc.BANDED_W for m in (w + 1,)}
    assert classes == {4, 8, 16, 32}
    assert {w + 1 for w in fc.BANDED_W} >= {4, 5, 8, 9, 16, 17, 32}                  # both sides of every class edge
    assert np.diff(cases["pattern16x16"]["G"][0]).max() == 7
    gp, gc, gv = cases["diagonal"]["G"]
    assert np.array_equal(gc, np.arange(len(gv))) and np.allclose(gv, cases["diagonal"]["vals"] ** -0.5, rtol=4e-16, atol=0)
    for name, c in cases.items():                                                      # lower triangular, diagonal last and positive
        gp, gc, gv = c["G"]
        last = gp[1:] - 1
        assert np.array_equal(gc[last], np.arange(len(gp) - 1)) and np.all(gv[last] > 0), name
        assert np.all(gc <= np.repeat(np.arange(len(gp) - 1), np.diff(gp))), name


def test_diagonal_of_GAGt_is_one(cases):
    for name, c in cases.items():
        d = float(np.max(np.abs(fc.diag_gagt(c["rowptr"], c["colidx"], c["vals"], c["G"]) - 1.0)))
        print(f"{name}: max |diag(G A G') - 1| = {d:.2e}")
        assert d <= fc.DIAG_ONE_TOL, name


def test_pcg_op_converges_on_every_spd_case(cases):
    for name, c in cases.items():
        x, its, status, h = fc.pcg_op(c["rowptr"], c["colidx"], c["vals"], c["b"], c["G"], rtol=1e-8)
        true = np.linalg.norm(c["b"] - pc.matvec(c["rowptr"], c["colidx"], c["vals"], x)) / np.linalg.norm(c["b"])
        print(f"{name}: {its} iterations, true residual {true:.2e}")
        assert status == "converged" and len(h) == its + 1, name
        assert true <= pc.TRUE_RES_RTOL, (name, true)
    assert fc.pcg_op(*[cases["diagonal"][k] for k in ("rowptr", "colidx", "vals", "b", "G")])[1] == 1


@pytest.mark.parametrize("size", pc.SIZES)
def test_pcg_op_beats_jacobi_on_the_scaled_cases(orc, size):
    nx, ny = size
    rowptr, colidx, vals, b = pc.scaled_poisson(orc, nx, ny)
    jacobi = pc.pcg(rowptr, colidx, vals, b, dinv=1.0 / pc.host_diag(rowptr, colidx, vals), rtol=1e-8)[1]
    checked = 0
    for k in fc.BLOCKS:
        G = fc.fsai_blocks(rowptr, colidx, vals, fc.equal_blocks(nx * ny, k))
        _, its, status, _ = fc.pcg_op(rowptr, colidx, vals, b, G, rtol=1e-8)
        print(f"{nx}x{ny}, {k} blocks: {its} iterations against Jacobi's {jacobi}: {its / jacobi:.3f}")
        assert status == "converged"
        if (size, k) in fc.JACOBI_SKIPPED:
            continue
        assert its <= fc.JACOBI_FACTOR * jacobi, (size, k, its, jacobi)
        checked += 1
    assert checked == len(fc.BLOCKS) - sum(1 for s, _ in fc.JACOBI_SKIPPED if s == size)


def test_the_failing_cases_fail_in_the_restatement():
    for factor in (fc.fsai_cholesky, fc.fsai_solve):
        for (mat, row) in (fc.not_spd_diag(), fc.not_spd_block()):
            with pytest.raises(fc.NotPositiveDefinite) as e:
                factor(*mat)
            assert e.value.row == row
        mat, row = fc.no_diagonal()
        with pytest.raises(fc.NoDiagonal) as e:
            factor(*mat)
        assert e.value.row == row
    assert np.diff(fc.fsai_cholesky(*fc.banded(fc.CAP_W))[0]).max() == 33            # over the cap of 32


def test_blocked_G_ignores_the_columns_of_other_blocks(orc):
    rowptr, colidx, vals, _ = pc.scaled_poisson(orc, 16, 16)
    part = fc.equal_blocks(256, 3)
    gp, gc, gv = fc.fsai_blocks(rowptr, colidx, vals, part)
    row_of = np.repeat(np.arange(256), np.diff(gp))
    owner = np.searchsorted(part, row_of, side="right") - 1
    assert np.all(gc >= np.asarray(part)[owner]) and np.all(gc <= row_of)
    # a block's first row stands alone; the next one keeps its left neighbour and loses the one above, which another block owns
    assert part[1] % 16 not in (0, 15) and np.diff(gp)[part[1]] == 1 and np.diff(gp)[part[1] + 1] == 2
    # an empty block is legal
    gp0, _, _ = fc.fsai_blocks(rowptr, colidx, vals, [0, 100, 100, 256])
    assert gp0[-1] == len(fc.fsai_blocks(rowptr, colidx, vals, [0, 100, 256])[1])


# ---- the hand-built inputs of the kernel tests --------------------------------------------------------------------------------
def test_three_faults_fail_in_row_order_and_heal_one_at_a_time():
    """The restatement walks the rows in order, so it names the smallest faulty row, as the device's error word must."""
    want = [(fc.NotPositiveDefinite, 40), (fc.NoDiagonal, 300), (fc.NotPositiveDefinite, 520)]
    assert tuple(r for _, r in want) == fc.FAULT_ROWS
    for heal, (exc, row) in enumerate(want):
        rowptr, colidx, vals = fc.three_faults(heal)
        assert len(rowptr) == 601 and rowptr[-1] == len(colidx) == len(vals)
        with pytest.raises(exc) as e:
            fc.fsai_cholesky(rowptr, colidx, vals)
        assert e.value.row == row, (heal, e.value.row)
    rowptr, colidx, vals = fc.three_faults(3)
    clean = fc.banded(3, 600)
    assert all(np.array_equal(a, b) for a, b in zip((rowptr, colidx, vals), clean))
    fc.fsai_cholesky(rowptr, colidx, vals)
    r, c, v = fc.three_faults(2)                                   # the last fault is a POSITIVE diagonal: only the pivot fails
    assert v[r[520] + np.flatnonzero(c[r[520]:r[521]] == 520)[0]] > 0


def test_pattern_is_not_a_has_the_three_kinds_of_entry_and_thins_to_the_same_G():
    import tests._amg_cases as ac
    A, P, Pthin, part, j = fc.pattern_is_not_a()
    lo, hi = part[j], part[j + 1]
    assert hi - lo == 40
    above = ghosts_in_front = unstored = outside = no_diag = 0
    for i in range(lo, hi):
        prow = P.indices[P.indptr[i]:P.indptr[i + 1]]
        arow = A.indices[A.indptr[i]:A.indptr[i + 1]]
        above += int(np.sum(prow > i))
        ghosts_in_front += int(prow[0] < lo)
        unstored += len(set(prow[(prow >= lo) & (prow < i)]) - set(arow))
        outside += len(set(arow[(arow >= lo) & (arow < i)]) - set(prow))
        no_diag += int(i not in prow)
    assert min(above, ghosts_in_front, unstored, outside, no_diag) >= 10
    _, split, _, n_own, _ = ac.split_block(P, part, j)
    rowptr = P.indptr[lo:hi + 1] - P.indptr[lo]
    assert np.sum(split[rowptr[:-1]] >= n_own) == ghosts_in_front    # in split form too the row opens with the ghost
    cut = lambda M: (M.indptr[lo:hi + 1] - M.indptr[lo], M.indices[M.indptr[lo]:M.indptr[hi]])
    rows = (*cut(A), A.data[A.indptr[lo]:A.indptr[hi]])
    full = fc.fsai_cholesky(*rows, row_start=lo, pattern=cut(P))
    thin = fc.fsai_cholesky(*rows, row_start=lo, pattern=cut(Pthin))
    own = fc.fsai_cholesky(*rows, row_start=lo)
    assert all(np.array_equal(a, b) for a, b in zip(full[:2], thin[:2])) and np.array_equal(pc.bits(full[2]), pc.bits(thin[2]))
    assert not np.array_equal(full[0], own[0])                      # and it is not the G of A's own pattern
    assert Pthin.nnz < P.nnz
