"""CPU checks of what tests/test_gpu_special_values.py feeds the GPU (tests/_special_values_cases.py), against the oracle
alone: the structures have the rows and columns their description claims, and the EXPECTED values hold every class of
result in every operand column, so the fixture cannot silently degenerate into finite data (or into all-NaN data)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _special_values_cases as sv  # noqa: E402

TYPES = [np.float64, np.float32]


def test_general_structure():
    rowptr, col = sv.general()
    n = len(rowptr) - 1
    ln = np.diff(rowptr)
    assert n == sv.NROWS and rowptr[0] == 0 and rowptr[-1] == len(col) and col.min() == 0 and col.max() == sv.NCOLS - 1
    for r in range(n):
        assert np.all(np.diff(col[rowptr[r]:rowptr[r + 1]]) > 0)               # ascending, duplicate-free
    assert {465, 1500, 2049, 3000} <= set(ln.tolist()) and np.all(ln[list(sv.EMPTY)] == 0) and len(sv.EMPTY) == 10
    assert np.median(ln) <= 11
    per_col = np.bincount(col, minlength=sv.NCOLS)
    assert per_col[sv.DENSE_COL] == (ln > 0).sum() > 1024                       # one column in every non-empty row
    assert per_col[0] >= 20 and per_col[-1] >= 20                                # column 0 and the last one are really read


def test_banded_structure_is_the_oracles_five_point_matrix(orc):
    rowptr, col, vals = sv.banded()
    rows = orc.poisson2d_rows(sv.NX, sv.NY, 0, sv.NX * sv.NY)
    assert sv.NX >= 256 and sv.NY >= 130
    np.testing.assert_array_equal(rowptr, rows.rowptr)
    np.testing.assert_array_equal(col, rows.colidx)
    np.testing.assert_array_equal(vals, rows.vals)


@pytest.mark.parametrize("T", TYPES)
def test_values_and_operand_hold_every_special(T):
    rowptr, col = sv.general()
    vals = sv.values(rowptr, col, T)
    assert vals.dtype == T
    tiny = np.finfo(T).tiny
    assert np.isnan(vals).sum() >= 4 and np.isposinf(vals).sum() >= 10 and np.isneginf(vals).sum() >= 10
    assert ((vals == 0) & np.signbit(vals)).sum() >= 30 and ((vals == 0) & ~np.signbit(vals)).sum() >= 30
    assert ((vals > 0) & (vals < tiny)).sum() >= 5                              # denormals
    for r, z in sv.ZERO_ROWS:
        seg = vals[rowptr[r]:rowptr[r + 1]]
        assert len(seg) >= 4 and np.all(seg == 0) and np.all(np.signbit(seg) == np.signbit(z))
    assert np.all(np.isfinite(vals[col == sv.DENSE_COL]))
    B = sv.operand(sv.NCOLS, 4, T)
    assert np.isposinf(B[:, 0]).sum() >= 30 and np.isneginf(B[:, 1]).sum() >= 30 and np.isnan(B[:, 2]).sum() >= 30
    assert ((B[:, 3] == 0) & np.signbit(B[:, 3])).sum() >= 30 and (B[:, 0] == np.finfo(T).max).sum() >= 30
    assert np.isposinf(B[0, 0]) and np.isposinf(B[-1, 0]) and np.isnan(B[0, 2]) and np.isnan(B[-1, 2])
    assert np.all(np.isfinite(B[sv.DENSE_COL]))
    Bc = sv.operand(sv.NCOLS, 4, T, rule="C")
    assert not (np.abs(Bc[np.isfinite(Bc)].astype(np.float64)) > 1e150).any() and not (Bc == np.finfo(T).max).any()


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("which", ["general", "banded"])
def test_expected_values_hold_every_class_in_every_column(orc, T, which):
    if which == "general":
        rowptr, col = sv.general()
        vals = sv.values(rowptr, col, T)
        ncols = sv.NCOLS
    else:
        rowptr, col, base = sv.banded()
        vals = sv.values(rowptr, col, T, base=base)
        ncols = sv.NX * sv.NY
    B = sv.operand(ncols, 4, T)
    with np.errstate(all="ignore"):
        want = orc.spmm(rowptr.astype(np.int32), col.astype(np.int32), vals, B)
    assert want.dtype == T
    for c in range(4):
        w = want[:, c]
        assert np.isnan(w).any() and np.isposinf(w).any() and np.isneginf(w).any(), (c, "non-finite classes")
        assert (w == 0).any() and (np.isfinite(w) & (w != 0)).any(), (c, "zero / finite")
    finite_nonzero = np.isfinite(want) & (want != 0)
    assert finite_nonzero.sum() >= want.size // 2
    assert not np.signbit(want[want == 0]).any()              # the loop starts from zero(T): it cannot produce -0.0
    # the all -0.0 rows: every product is -0.0 (the operand is positive where they read), the sum from zero(T) is +0.0 -- a
    # kernel that starts from its first product gives -0.0 there
    for r, z in (sv.ZERO_ROWS if which == "general" else sv.ZERO_ROWS_BANDED):
        if np.signbit(z):
            seg = slice(rowptr[r], rowptr[r + 1])
            prod = vals[seg, None] * B[col[seg]]
            assert np.all(prod == 0) and np.all(np.signbit(prod)) and np.all(want[r] == 0) and not np.signbit(want[r]).any()


def test_oracle_is_the_plain_loop_on_special_values(orc):
    """The expected values themselves: the oracle's row sums equal a Python loop (acc = 0; acc += a * b) on rows that hold
    specials -- NaN compared as NaN, zero with its sign."""
    rowptr, col = sv.general()
    vals = sv.values(rowptr, col, np.float64)
    B = sv.operand(sv.NCOLS, 4, np.float64)
    with np.errstate(all="ignore"):
        want = orc.spmm(rowptr.astype(np.int32), col.astype(np.int32), vals, B)
        for r in [10, 11, 701, 5, 63, 0, 37, 41, 300] + list(range(400, 440)):
            acc = np.zeros(4)
            for j in range(rowptr[r], rowptr[r + 1]):
                acc = acc + vals[j] * B[col[j]]
            np.testing.assert_array_equal(want[r], acc)
            z = acc == 0
            assert np.array_equal(np.signbit(want[r][z]), np.signbit(acc[z]))


def test_classes_of_products_match_the_sequential_sum(orc):
    """Rule C's class function against the oracle's sequential sum on the rule-C operands (no finfo.max: no overflow)."""
    rowptr, col = sv.general()
    vals = sv.values(rowptr, col, np.float64)
    x = sv.operand(sv.NCOLS, 4, np.float64, rule="C")
    for c in range(4):
        with np.errstate(all="ignore"):
            y = orc.spmv(rowptr.astype(np.int32), col.astype(np.int32), vals, np.ascontiguousarray(x[:, c]))
        cls, ref, bound = sv.csr_classes(rowptr, col, vals, x[:, c])
        np.testing.assert_array_equal(sv.class_of_values(y), cls)
        fin = cls == sv.FINITE
        assert np.all(np.abs(y[fin] - ref[fin]) <= 1e-12 * bound[fin])
    assert sv.classes_of(np.array([[1.0, np.inf, np.inf, np.nan], [2.0, 3.0, -np.inf, np.inf]])).tolist() == \
        [sv.FINITE, sv.PINF, sv.NAN, sv.NAN]


def test_transpose_csr_keeps_row_order_within_a_column():
    rowptr, col = sv.general()
    vals = np.arange(len(col), dtype=np.float64)
    t_rp, t_row, t_val = sv.transpose_csr(rowptr, col, vals, sv.NCOLS)
    assert t_rp[-1] == len(col) and len(t_rp) == sv.NCOLS + 1
    seg = slice(t_rp[sv.DENSE_COL], t_rp[sv.DENSE_COL + 1])
    assert np.all(np.diff(t_row[seg]) > 0) and seg.stop - seg.start > 1024
    j = int(t_rp[sv.DENSE_COL]) + 7
    r = int(t_row[j])
    assert col[int(t_val[j])] == sv.DENSE_COL and rowptr[r] <= int(t_val[j]) < rowptr[r + 1]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("rule", ["E", "C"])
@pytest.mark.parametrize("k", [1, 3, 4, 16])
def test_long_rows_have_their_placed_classes(orc, T, rule, k):
    """The rows that reach the kernels' multi-pass code (465 ... 3 000 entries) must not all be NaN, or those passes could add
    0 * Inf, start from the first product or drop a pass unnoticed: every long row has the class LONG_CLASS names, in every
    operand column, for both rules -- finite non-zero, an exact +0.0 from -0.0 products, +Inf, -Inf and NaN all occur."""
    rowptr, col = sv.general()
    ln = np.diff(rowptr)
    assert sorted(np.flatnonzero(ln >= 465).tolist()) == sorted(sv.LONG) and all(ln[r] == l for r, l in sv.LONG.items())
    vals = sv.values(rowptr, col, T)
    B = sv.operand(sv.NCOLS, k, T, rule=rule)
    assert np.all(np.isfinite(B[sv.BAND[0]:sv.BAND[1]])) and np.all(B[sv.BAND[0]:sv.BAND[1]] != 0)
    with np.errstate(all="ignore"):
        want = orc.spmm(rowptr.astype(np.int32), col.astype(np.int32), vals, B)
    for r, cls in sv.LONG_CLASS.items():
        assert np.all(sv.class_of_values(want[r]) == cls), (r, want[r])
        for c in range(k):
            assert sv.csr_classes(rowptr, col, vals, B[:, c])[0][r] == cls
    assert np.all(want[[5, 63]] != 0) and np.all(want[901] == 0) and not np.signbit(want[901]).any()
    seg = slice(rowptr[901], rowptr[902])
    assert np.all(np.signbit(vals[seg, None] * B[col[seg]]))                 # every product of the long zero row is -0.0
    tiny, big = np.finfo(T).tiny, np.finfo(T).max
    row5 = vals[rowptr[5]:rowptr[6]]
    assert (row5 == big).sum() == 1 and ((row5 > 0) & (row5 < tiny)).sum() == 2 and (row5 == 0).sum() == 2
    long_rows_63_up = np.concatenate([vals[rowptr[r]:rowptr[r + 1]] for r in sv.LONG if sv.LONG[r] >= 928])
    assert not (np.abs(long_rows_63_up[np.isfinite(long_rows_63_up)]) == big).any()      # rule C rows: no finfo.max


@pytest.mark.parametrize("m", [2, 16, 17, 64])
def test_transposed_product_over_the_dense_column_has_one_class_per_operand_column(orc, m):
    """transpose(X) * A: the sum over the column present in every row (> 1 024 entries, several passes) is +Inf, -Inf, NaN or
    finite according to the operand column's special, not NaN throughout."""
    rowptr, col = sv.general()
    vals = sv.values(rowptr, col, np.float64)
    t_rp, t_row, t_val = sv.transpose_csr(rowptr, col, vals, sv.NCOLS)
    X = sv.operand(sv.NROWS, m, np.float64, per=12, ordinary=[r for r, _ in sv.ZERO_ROWS])     # no 0 * Inf in that column
    with np.errstate(all="ignore"):
        W = orc.spmm(t_rp.astype(np.int32), t_row.astype(np.int32), t_val, X)
    got = sv.class_of_values(W[sv.DENSE_COL])
    assert got.tolist() == [(sv.PINF, sv.NINF, sv.NAN, sv.FINITE)[c % 4] for c in range(m)]
