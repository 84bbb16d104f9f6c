"""CPU checks of what tests/test_gpu_narrow_cols.py feeds the GPU: the generated matrices have the properties their names
claim, the numpy eligibility rule says what the issue's rule says, block-relative int16 deltas decode back to the columns
(the kernel's r0 + d), and the oracle's product over these matrices is the plain stored-order sum.  Also the host switch."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _narrow_cols_cases import HI, LO, PASS, RPB, banded_edges, eligible_np, long_and_empty_rows, tail_case  # noqa: E402


def _check_csr(rowptr, col, vals):
    n = len(rowptr) - 1
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(vals) and np.all(np.diff(rowptr) >= 0)
    assert col.min() >= 0 and col.max() < n and np.all(np.isfinite(vals)) and np.all(vals != 0)
    for r in range(n):
        seg = col[rowptr[r]:rowptr[r + 1]]
        assert np.all(np.diff(seg) > 0)
    return n


def _roundtrip(rowptr, col):
    """int16 block-relative deltas and back: what hpcla_cols16_encode_i32 stores and IndexPolicy<Cols16>::decode reads."""
    n = len(rowptr) - 1
    r0 = RPB * (np.repeat(np.arange(n), np.diff(rowptr)) // RPB)
    d = (col - r0).astype(np.int16)
    return np.array_equal(r0 + d.astype(np.int64), col)


@pytest.mark.parametrize("which,expect", [("edges", True), ("past_low", False), ("past_high", False)])
def test_banded_edges(which, expect):
    rowptr, col, vals = banded_edges(which)
    n = _check_csr(rowptr, col, vals)
    assert eligible_np(rowptr, col, n) == expect
    assert _roundtrip(rowptr, col) == expect                 # past an edge the int16 wraps: exactly why such a plan falls back
    r0 = 128 * RPB
    seg = col[rowptr[r0]:rowptr[r0 + RPB]] - r0
    assert seg.min() == LO and seg.max() == HI               # both extreme deltas in ONE block
    if not expect:
        r1 = 129 * RPB
        seg = col[rowptr[r1]:rowptr[r1 + RPB]] - r1
        assert (seg.min() == LO - 1) != (seg.max() == HI + 1)
        assert eligible_np(rowptr, col, n, blocks=[b for b in range((n + RPB - 1) // RPB) if b != 129])
    assert not eligible_np(rowptr, col, n_own=65535)         # a ghost column (>= n_own) disqualifies the block that holds it


def test_long_and_empty_rows():
    rowptr, col, vals = long_and_empty_rows()
    n = _check_csr(rowptr, col, vals)
    ln = np.diff(rowptr)
    assert eligible_np(rowptr, col, n) and _roundtrip(rowptr, col)
    assert {465, 2 * PASS, PASS, 1500, 3000} <= set(ln.tolist()) and (ln == 0).sum() > 300
    assert np.all(ln[256:300] == 0) and np.all(ln[1280:1500] == 0)       # an empty wave, an empty block
    # at least one pass of a wave lies wholly inside one row (the kernel's whole-pass branch): row 1024 is the first row of its
    # wave, so its passes start at its first entry rounded down to a multiple of 8
    p0, p1 = int(rowptr[1024]), int(rowptr[1025])
    pa = p0 & ~7
    assert any(pa + c >= p0 and pa + c + PASS <= p1 for c in range(0, p1 - pa, PASS))


@pytest.mark.parametrize("short", range(8))
def test_tail_case(short):
    rowptr, col, vals = tail_case(short)
    n = _check_csr(rowptr, col, vals)
    assert eligible_np(rowptr, col, n) and _roundtrip(rowptr, col)
    assert (8 - len(col) % 8) % 8 == short


def test_oracle_product_of_a_case_is_the_stored_order_sum():
    from oracle import oracle as orc
    rowptr, col, vals = long_and_empty_rows()
    n = len(rowptr) - 1
    x = orc.fill_uniform(0, n, orc.SEED_X) - 0.5
    y = orc.spmv(rowptr.astype(np.int32), col.astype(np.int32), vals, x)
    for r in (5, 6, 71, 300, 1024, 2999, 0):
        acc = 0.0
        for j in range(rowptr[r], rowptr[r + 1]):
            acc += vals[j] * x[col[j]]
        assert y[r] == acc


def test_switch_reads_like_the_index_narrowing_switch(monkeypatch):
    from hpcla_amd import sparse
    monkeypatch.delenv("HPCLA_NARROW_COLS", raising=False)
    assert sparse.narrow_cols_enabled()
    for v in ("0", "off", "False", " no "):
        monkeypatch.setenv("HPCLA_NARROW_COLS", v)
        assert not sparse.narrow_cols_enabled()
    monkeypatch.setenv("HPCLA_NARROW_COLS", "1")
    assert sparse.narrow_cols_enabled()


def test_kernel_keeps_four_template_parameters_and_one_body():
    """The narrow form is an index POLICY of spmv_rowgather_kernel, not a copy of its body."""
    text = open(os.path.join(ROOT, "linearalgebrampi.jl_amd", "csrc", "spmv.hip")).read()
    assert text.count("void spmv_rowgather_kernel(") == 1
    assert "spmv_rowgather_kernel<Cols16, false, false>" in text and "struct IndexPolicy<Cols16>" in text
