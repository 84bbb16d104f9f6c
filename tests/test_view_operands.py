"""The view-operand helpers keep what their names promise (tests/_view_operands.py), on CPU tensors: the offset arithmetic is
the same on a device, where tests/test_gpu_view_operands.py asserts it again before every call."""
import numpy as np
import pytest
import torch

from tests import _view_operands as vo

VEC_N = (1, 2, 3, 257, 2051)
MAT_NK = [(n, k) for n in (1, 65, 257) for k in (1, 2, 3, 8, 16, 17)]


def _poison_outside(buf, op):
    """Every element of the buffer that the operand does not cover is still NaN."""
    mask = torch.ones(buf.numel(), dtype=torch.bool)
    first = (op.data_ptr() - buf.data_ptr()) // buf.element_size()
    idx = first + sum(torch.arange(s).reshape([-1 if d == e else 1 for e in range(op.dim())]) * st
                      for d, (s, st) in enumerate(zip(op.shape, op.stride())))
    mask[idx.reshape(-1)] = False
    return bool(torch.isnan(buf[mask]).all()) and int(mask.sum()) == buf.numel() - op.numel()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", VEC_N)
def test_vector_variants_keep_their_promise(dtype, n):
    values = np.random.default_rng(n).standard_normal(n).astype(dtype)
    for variant in vo.vector_variants(dtype):
        buf, op = vo.place_vector(values, variant)
        assert buf.data_ptr() % 16 == 0
        assert (op.data_ptr() % 16, op.is_contiguous()) == vo.vector_promise(variant, dtype), variant
        assert op.shape == (n,) and np.array_equal(op.numpy(), values), variant      # the values round-trip
        assert _poison_outside(buf, op), variant
        assert (variant == "fresh") == (buf.numel() == n)
        again = vo.vector_view(buf.clone(), variant, n)                              # the same cut of another buffer
        assert again.storage_offset() == op.storage_offset() and np.array_equal(again.numpy(), values)


def test_vector_variant_lists():
    assert vo.VECTOR_F64 == ("fresh", "off8", "chunk") and vo.VECTOR_F32 == ("fresh", "off4", "off8", "off12")
    assert {vo.vector_promise(v)[0] for v in vo.VECTOR_F32} == {0, 4, 8, 12}
    with pytest.raises(ValueError):
        vo.place_vector(np.zeros(4), "off4")                                         # half a double
    with pytest.raises(ValueError):
        vo.place_vector(np.zeros(4, dtype=np.float32), "chunk")


def test_chunk_is_the_second_piece_of_an_odd_split():
    for n in VEC_N:
        buf, op = vo.place_vector(np.arange(n, dtype=np.float64), "chunk")
        first, second = torch.chunk(buf, 2)
        assert first.numel() % 2 == 1 and second.data_ptr() == op.data_ptr() and second.numel() == n


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,k", MAT_NK)
def test_matrix_variants_keep_their_promise(dtype, n, k):
    values = np.random.default_rng(n * 100 + k).standard_normal((n, k)).astype(dtype)
    for variant in vo.MATRIX:
        buf, op = vo.place_matrix(values, variant)
        assert buf.data_ptr() % 16 == 0
        assert (op.data_ptr() % 16, op.is_contiguous()) == vo.matrix_promise(variant, n, k, dtype), variant
        assert op.shape == (n, k) and np.array_equal(op.numpy(), values), variant
        assert _poison_outside(buf, op), variant
        again = vo.matrix_view(buf.clone(), variant, n, k)
        assert again.stride() == op.stride() and again.storage_offset() == op.storage_offset()
    pitches = {v: vo.place_matrix(values, v)[1].stride() for v in vo.MATRIX}
    assert pitches["pitch_odd"] == (k + 1, 1) and pitches["pitch_even"] == (k + 2, 1) and pitches["col_off1"] == (k + 2, 1)
    assert pitches["colmajor"] == (1, n) and pitches["fresh"] == pitches["off8"] == (k, 1)
    if n > 1:                              # the names' contiguity, where torch's definition leaves a choice
        assert not any(vo.matrix_promise(v, n, k)[1] for v in ("pitch_odd", "pitch_even", "col_off1"))
        assert vo.matrix_promise("colmajor", n, k)[1] == (k == 1)


def test_combos_vary_each_position_alone_then_all_together():
    c = vo.combos(vo.VECTOR_F64, vo.VECTOR_F64)
    assert c == [("fresh", "fresh"), ("off8", "fresh"), ("chunk", "fresh"), ("fresh", "off8"), ("fresh", "chunk"),
                 ("off8", "off8"), ("off8", "chunk"), ("chunk", "off8"), ("chunk", "chunk")]
    assert vo.combos(vo.VECTOR_F32) == [(v,) for v in vo.VECTOR_F32]
    four = vo.combos(*[vo.VECTOR_F64] * 4)
    assert len(four) == len(set(four)) == 1 + 4 * 2 + 2 ** 4
    mixed = vo.combos(vo.MATRIX, vo.VECTOR_F64)
    assert len(mixed) == 1 + 5 + 2 + 5 * 2 and ("col_off1", "chunk") in mixed and ("fresh", "off8") in mixed
