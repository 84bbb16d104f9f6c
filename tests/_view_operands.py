"""Operands that are views: given values placed inside a larger NaN-poisoned buffer, at the offsets and pitches a caller's own
storage can have.  ``HPCVector_local`` / ``HPCMatrix(...)`` keep such a tensor as it is, so its device pointer reaches the C ABI
unchanged; the vector kernels there work in 16-byte accesses.

Every placement returns ``(whole buffer, operand)``; ``view(buf, ...)`` cuts the same operand out of another buffer of the same
size (a snapshot, an expected image).  ``promise(...)`` is what a variant's name says about the operand: ``(data_ptr() % 16,
is_contiguous())``.  The offset arithmetic is the same on the CPU and on a device (both allocators return blocks aligned to at
least 64 bytes), which tests/test_view_operands.py asserts on CPU tensors.  No device is needed to import this module.
"""
import numpy as np

VECTOR_F64 = ("fresh", "off8", "chunk")
VECTOR_F32 = ("fresh", "off4", "off8", "off12")
MATRIX = ("fresh", "off8", "pitch_odd", "pitch_even", "col_off1", "colmajor")


def vector_variants(dtype):
    return VECTOR_F32 if np.dtype(dtype) == np.float32 else VECTOR_F64


def _torch():
    import torch
    return torch


def _tdtype(dtype):
    torch = _torch()
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def _poison(numel, dtype, device):
    torch = _torch()
    return torch.full((int(numel),), float("nan"), dtype=_tdtype(dtype), device=device)


def bits(t):
    """The tensor's bit patterns as integers (NaN poison compares equal to itself)."""
    torch = _torch()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- vectors -----------------------------------------------------------------------------------------------------------------------
def _vector_span(variant, n, dtype):
    """(buffer length, first element of the operand) of a vector variant."""
    item = np.dtype(dtype).itemsize
    if variant == "fresh":
        return n, 0
    if variant == "chunk":                                       # two pieces of an ODD length p >= n; the operand is the second
        p = n if n % 2 else n + 1
        if item == 4:
            raise ValueError("chunk is a float64 variant")
        return p + n, p
    lead = {"off4": 4, "off8": 8, "off12": 12}[variant]
    if lead % item:
        raise ValueError(f"{variant} is not a whole number of {np.dtype(dtype).name} elements")
    return n + 16 // item, lead // item                          # 16 bytes of poison shared between the two ends


def vector_view(buf, variant, n):
    dtype = np.float32 if buf.element_size() == 4 else np.float64
    total, first = _vector_span(variant, n, dtype)
    assert buf.numel() == total
    if variant == "chunk":
        piece = _torch().chunk(buf, 2)[1]
        assert piece.numel() == n and piece.storage_offset() == first
        return piece
    return buf[first:first + n]


def vector_promise(variant, dtype=np.float64):
    """(data_ptr() % 16, is_contiguous()) of a vector variant."""
    return {"fresh": 0, "off4": 4, "off8": 8, "off12": 12, "chunk": 8}[variant], True


def place_vector(values, variant, device="cpu"):
    """``values`` (a 1-D numpy array, float64 or float32) as the named view: (whole buffer, operand)."""
    torch = _torch()
    values = np.array(values)                                    # a writable copy: torch.from_numpy wants one
    n = len(values)
    total, _ = _vector_span(variant, n, values.dtype)
    buf = _poison(total, values.dtype, device)
    op = vector_view(buf, variant, n)
    op.copy_(torch.from_numpy(values))
    return buf, op


# ---- (n, k) blocks -----------------------------------------------------------------------------------------------------------------
def _matrix_span(variant, n, k, dtype):
    item = np.dtype(dtype).itemsize
    if variant == "fresh":
        return n * k
    if variant == "off8":
        return n * k + 16 // item
    if variant == "pitch_odd":
        return n * (k + 1)
    if variant == "pitch_even":
        return n * (k + 2)
    if variant == "col_off1":
        return n * (k + 2)
    if variant == "colmajor":
        return n * k
    raise ValueError(variant)


def matrix_view(buf, variant, n, k):
    item = buf.element_size()
    assert buf.numel() == _matrix_span(variant, n, k, np.float32 if item == 4 else np.float64)
    if variant == "fresh":
        return buf.view(n, k)
    if variant == "off8":
        return buf[8 // item:8 // item + n * k].view(n, k)
    if variant == "pitch_odd":
        return buf.view(n, k + 1)[:, :k]
    if variant == "pitch_even":
        return buf.view(n, k + 2)[:, :k]
    if variant == "col_off1":
        return buf.view(n, k + 2)[:, 1:1 + k]
    return buf.view(k, n).t()                                    # colmajor


def matrix_promise(variant, n, k, dtype=np.float64):
    """(data_ptr() % 16, is_contiguous()) of a block variant.  torch calls a block contiguous whenever no stride that matters
    differs from the packed one, so a one-row slice of a wider buffer and a transposed block with n = 1 or k = 1 are."""
    item = np.dtype(dtype).itemsize
    mod = {"off8": 8, "col_off1": item}.get(variant, 0)
    if variant in ("fresh", "off8"):
        return mod, True
    if variant == "colmajor":
        return mod, n == 1 or k == 1
    return mod, n == 1


def place_matrix(values, variant, device="cpu"):
    """``values`` (an (n, k) numpy array) as the named view: (whole buffer, operand)."""
    torch = _torch()
    values = np.array(values)
    n, k = values.shape
    buf = _poison(_matrix_span(variant, n, k, values.dtype), values.dtype, device)
    op = matrix_view(buf, variant, n, k)
    op.copy_(torch.from_numpy(values))
    return buf, op


def combos(*variants_of_position):
    """The sweep over operand positions, one list of variant names per position (each list starts with "fresh"): every
    position alone over all its variants while the others stay fresh, then all positions off "fresh" together, in every
    combination of their non-fresh variants.  Tuples of variant names, one per position, without repeats."""
    import itertools
    lists = [tuple(v) for v in variants_of_position]
    assert all(v[0] == "fresh" for v in lists)
    seen, out = set(), []

    def add(c):
        if c not in seen:
            seen.add(c)
            out.append(c)
    for p, mine in enumerate(lists):
        for v in mine:
            add(tuple(v if q == p else "fresh" for q in range(len(lists))))
    for c in itertools.product(*(v[1:] for v in lists)):
        add(tuple(c))
    return out
