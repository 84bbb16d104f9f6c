"""CPU checks of what tests/test_gpu_block_patterns.py feeds the GPU: the numpy model of the pattern rule counts what the
issue counted (18 patterns for the 4096-wide 5-point matrix, 36 for the 512 x 512 x 8 7-point one), the generated matrices
have the properties their names claim, and the host switch and the plan cache key read as documented."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _narrow_cols_cases import RPB, eligible_np, long_and_empty_rows, tail_case  # noqa: E402
from _block_patterns_cases import (CAP_BYTES, HEAD, band_with_random_half, model_table, more_patterns_than_the_cap,  # noqa: E402
                                   one_column_off, pattern_entries, pattern_keys_np, unstructured)
from test_narrow_cols_cases import _check_csr  # noqa: E402


def test_headline_matrix_has_18_patterns():
    from hpcla_amd import workloads
    rowptr, col, _ = workloads.poisson2d_rows(4096, 512, 0, 512 * 4096)
    keys = pattern_keys_np(rowptr, col)
    cnt = Counter(keys.values())
    assert len(keys) == 8192 and len(cnt) == 18
    assert sorted(cnt.values(), reverse=True)[:4] == [1792, 1792, 1778, 1778]
    assert int(np.abs(col - RPB * (np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)) // RPB)).max()) == 4351
    m = model_table(rowptr, col)
    assert m["patterns"] == 18 and m["patterned"] == 8192 and m["candidates"] == 8192
    assert 44_000 < m["table_bytes"] < 60_000 and m["table_bytes"] == 2 * sum(pattern_entries(k) for k in cnt)
    # the byte model of the 4096^2 headline: values, x and y, one 8-byte record per block; against cols16 + rowptr streamed
    N = 4096
    nnz, n = 5 * N * N - 4 * N, N * N
    assert 8 * nnz + 16 * n + 8 * (n // RPB) == 939_917_312 and 10 * nnz + 16 * n + 4 * (n + 1) == 1_174_241_284


def test_seven_point_slab_has_36_patterns_and_leaves_the_16_bit_window():
    from hpcla_amd import workloads
    rowptr, col, _ = workloads.poisson3d_rows(512, 512, 8, 0, 512 * 512 * 8)
    assert len(set(pattern_keys_np(rowptr, col).values())) == 36
    assert int(np.abs(col - RPB * (np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)) // RPB)).max()) == 262_399
    assert not eligible_np(rowptr, col, len(rowptr) - 1)


@pytest.mark.parametrize("nx,ny,ragged", [(4096, 24, False), (300, 300, True), (1000, 200, True), (512, 64, False)])
def test_five_point_grids(nx, ny, ragged):
    from hpcla_amd import workloads
    n = nx * ny
    rowptr, col, _ = workloads.poisson2d_rows(nx, ny, 0, n)
    assert (n % RPB != 0) == ragged
    keys = pattern_keys_np(rowptr, col)
    m = model_table(rowptr, col)
    assert m is not None and m["patterned"] == m["candidates"] == len(keys), "every pattern of these grids fits the table"
    if nx == 1000:
        assert len({k[0] for k in keys.values()}) >= 5, "the phases cycle (a block's first entry mod 8 takes many values)"
        assert nx % RPB != 0
    if ragged:
        assert keys[len(keys) - 1][1] == n % RPB


def test_small_seven_point_grid_fits_the_window():
    from hpcla_amd import workloads
    n = 32 * 32 * 40
    rowptr, col, _ = workloads.poisson3d_rows(32, 32, 40, 0, n)
    assert eligible_np(rowptr, col, n)
    m = model_table(rowptr, col)
    assert m is not None and m["patterned"] == m["candidates"] == n // RPB and m["patterns"] < m["candidates"] // 2


def test_band_with_random_half():
    rowptr, col, vals = band_with_random_half()
    n = _check_csr(rowptr, col, vals)
    assert eligible_np(rowptr, col, n)
    keys = pattern_keys_np(rowptr, col)
    cnt = Counter(keys.values())
    first, second = [keys[b] for b in range(64)], [keys[b] for b in range(64, 128)]
    assert max(cnt[k] for k in first) >= 8, "the stencil half repeats"
    assert all(cnt[k] == 1 for k in second), "no two blocks of the random half are alike"
    m = model_table(rowptr, col)
    assert m is not None and 64 <= m["patterned"] <= 128       # both kinds of block are candidates of ONE launch


def test_one_column_off():
    (rowptr, col, vals), blk = one_column_off()
    n = _check_csr(rowptr, col, vals)
    assert eligible_np(rowptr, col, n)
    keys = pattern_keys_np(rowptr, col)
    a, b = keys[blk - 1], keys[blk]
    assert a[:3] == b[:3] and a[3] != b[3], "same phase, rows and row lengths; other columns"
    da = np.frombuffer(a[3], dtype=np.int64)
    db = np.frombuffer(b[3], dtype=np.int64)
    assert int((da != db).sum()) == 1 and int(np.abs(da - db).max()) == 1
    assert Counter(keys.values())[a] == 37 and Counter(keys.values())[b] == 1
    m = model_table(rowptr, col)
    assert m["patterns"] == 4 and m["patterned"] == 40         # first block, last block, the common one, the odd one


def test_more_patterns_than_the_cap():
    (rowptr, col, vals), odd = more_patterns_than_the_cap()
    n = _check_csr(rowptr, col, vals)
    assert eligible_np(rowptr, col, n)
    cnt = Counter(pattern_keys_np(rowptr, col).values())
    assert sum(pattern_entries(k) for k in cnt) * 2 > CAP_BYTES, "all patterns together exceed the cap"
    assert sorted(cnt.values(), reverse=True)[:2] == [420 - len(odd) - 2, 1]
    m = model_table(rowptr, col)
    assert m is not None and m["patterns"] < len(cnt) and m["table_bytes"] <= CAP_BYTES
    assert m["table_bytes"] + 2 * (HEAD + 1280) > CAP_BYTES, "the table is full"
    assert 420 - len(odd) - 2 < m["patterned"] < 420, "the most frequent are kept, the rest stream"


def test_unstructured_gets_no_table():
    rowptr, col, vals = unstructured()
    n = _check_csr(rowptr, col, vals)
    assert eligible_np(rowptr, col, n)
    assert model_table(rowptr, col) is None


def test_small_cases_are_wholly_tabulated():
    """Every pattern of a small matrix fits the table, so the long-row / empty-row / tail cases run the pattern form."""
    for rowptr, col, _ in [long_and_empty_rows()] + [tail_case(s) for s in range(8)]:
        m = model_table(rowptr, col)
        assert m is not None and m["patterned"] == m["candidates"]


def test_switch_and_cache_key(monkeypatch):
    from hpcla_amd import sparse
    monkeypatch.delenv("HPCLA_NARROW_COLS", raising=False)
    monkeypatch.delenv("HPCLA_BLOCK_PATTERNS", raising=False)
    assert sparse.block_patterns_enabled()
    for v in ("0", "off", "False", " no "):
        monkeypatch.setenv("HPCLA_BLOCK_PATTERNS", v)
        assert not sparse.block_patterns_enabled() and sparse.narrow_cols_enabled()
    monkeypatch.setenv("HPCLA_BLOCK_PATTERNS", "1")
    assert sparse.block_patterns_enabled()
    monkeypatch.setenv("HPCLA_NARROW_COLS", "0")
    assert not sparse.block_patterns_enabled(), "HPCLA_NARROW_COLS=0 switches both off"

    class _A:
        T, Ti = np.dtype(np.float64), np.dtype(np.int32)
        _block_order_hint = 1

        def _ensure_hash(self):
            return b"a"

    class _X:
        structural_hash = b"x"

    seen = {}

    class _Plan:
        narrowed, block_group = False, 1

        def __init__(self, A, x):
            pass
    monkeypatch.setattr(sparse, "VectorPlan", _Plan)
    monkeypatch.setattr(sparse, "_vector_plan_cache", seen)
    for env in ({}, {"HPCLA_BLOCK_PATTERNS": "0"}, {"HPCLA_NARROW_COLS": "0"}, {"HPCLA_NARROW_COLS": "0", "HPCLA_BLOCK_PATTERNS": "0"}):
        monkeypatch.delenv("HPCLA_NARROW_COLS", raising=False)
        monkeypatch.delenv("HPCLA_BLOCK_PATTERNS", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sparse.get_vector_plan(_A(), _X())
    tags = sorted(k[5:] for k in seen)
    assert tags == [(), ("cols32",), ("nopat",)], "one plan per form; HPCLA_NARROW_COLS=0 needs no second tag"


def test_pattern_form_is_a_policy_of_the_one_kernel_body():
    text = open(os.path.join(ROOT, "linearalgebrampi.jl_amd", "csrc", "spmv.hip")).read()
    assert text.count("void spmv_rowgather_kernel(") == 1
    assert "struct IndexPolicy<Pat16> : IndexPolicy<Cols16>" in text and "spmv_rowgather_kernel<Pat16, false, false>" in text
