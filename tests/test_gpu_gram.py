"""transpose(X) * Y of two dense row-partitioned blocks (csrc/gram.hip, dense.dense_matmat_t) on the GPU.

* the reference's own fixture (test/test_new_operations.jl:109-113, B[i,j] = i + 0.1j, 8 x 6) through the public
  operator, against numpy, and exactly symmetric;
* integer-valued blocks (every partial sum exact): bit-equal to numpy's int64 product for every layout pair, padded
  leading dimensions, widths 1 .. 64 that are and are not multiples of 16, and row counts 0, 1, 63, 64, 65 and a large
  odd one;
* random blocks: the componentwise bound |C - C_ref| <= 1e-12 |X|^T |Y|, identical bits on a second call, X == Y
  exactly symmetric;
* Float32: every entry within 1 ulp of float32(exact);
* several ranks (tests/_multirank_gram_worker.py, one process per rank sharing the GPU): partitions and slices against
  the 1-rank product.
"""
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_gram_worker.py")

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 15, 16, 17, 31, 33, 64)


def _torch():
    import torch
    return torch


def _block(M, layout, pad, dtype):
    """(device tensor, leading dimension) holding the (n x w) block M in the given layout with `pad` spare entries per
    leading-dimension stride."""
    torch = _torch()
    n, w = M.shape
    if layout == "row":
        ld = w + pad
        buf = np.full((n, ld), 7.0, dtype=dtype)
        buf[:, :w] = M
    else:
        ld = n + pad
        buf = np.full((w, ld), 7.0, dtype=dtype)
        buf[:, :n] = M.T
    return torch.from_numpy(buf).cuda(), ld


def _gram_raw(hp, X, Y, xl="row", yl="row", xpad=0, ypad=0, dtype=np.float64, same=False):
    """C (m x k, double) of the local product through the C ABI, no communicator."""
    torch = _torch()
    from hpcla_amd.vectors import current_stream_ptr, dptr
    n, m = X.shape
    k = Y.shape[1]
    Xd, ldx = _block(X, xl, xpad, dtype)
    Yd, ldy = (Xd, ldx) if same else _block(Y, yl, ypad, dtype)
    lay = {"row": hp._capi.LAYOUT_ROW, "col": hp._capi.LAYOUT_COL}
    C = torch.full((max(m, 1), max(k, 1)), float("nan"), dtype=torch.float64, device="cuda")
    wb = hp._capi.load().hpcla_gram_work_bytes(n, m, k)
    work = torch.empty(max(1, wb // 8), dtype=torch.float64, device="cuda")
    sfx = "f32" if dtype == np.float32 else "f64"
    hp._capi.call(f"hpcla_gram_{sfx}", None, dptr(Xd), ldx, lay[xl], dptr(Yd), ldy, lay[yl if not same else xl], n, m, k,
                  dptr(C), dptr(work), current_stream_ptr())
    torch.cuda.synchronize()
    return C.cpu().numpy()[:m, :k]


def _ints(rng, n, w):
    return rng.integers(-8, 9, size=(n, w)).astype(np.int64)


def test_reference_fixture_through_the_operator(hp):
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    Bg = np.array([[i + 0.1 * j for j in range(1, 7)] for i in range(1, 9)], dtype=np.float64)
    Bm = hp.HPCMatrix.from_global(Bg, backend)
    G = hp.transpose(Bm) @ Bm
    assert isinstance(G, hp.HPCMatrix)
    got = G.gather()
    want = Bg.T @ Bg
    assert got.shape == (6, 6)
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want))
    assert np.array_equal(got, got.T)
    assert np.array_equal(G.row_partition, Bm.col_partition)
    assert np.array_equal(G.col_partition, hp.uniform_partition(6, 1))
    # the named entry, and a second block
    Yg = Bg[:, :4] * 2.0 - 1.0
    Y = hp.HPCMatrix.from_global(Yg, backend)
    G2 = hp.dense_matmat_t(Bm, Y)
    want2 = Bg.T @ Yg
    assert np.all(np.abs(G2.gather() - want2) <= 1e-12 * (np.abs(Bg).T @ np.abs(Yg)))
    with pytest.raises(ValueError, match="dimension mismatch"):
        hp.transpose(Bm) @ hp.HPCMatrix.from_global(Bg[:5], backend)


@pytest.mark.parametrize("m", WIDTHS)
def test_integer_blocks_bit_equal_every_width(hp, m):
    rng = np.random.default_rng(100 + m)
    n = 1237
    X = _ints(rng, n, m)
    for k in WIDTHS:
        Y = _ints(rng, n, k)
        got = _gram_raw(hp, X.astype(np.float64), Y.astype(np.float64))
        assert np.array_equal(got, (X.T @ Y).astype(np.float64)), (m, k)


@pytest.mark.parametrize("xl,yl", [("row", "row"), ("row", "col"), ("col", "row"), ("col", "col")])
def test_integer_blocks_bit_equal_every_layout(hp, xl, yl):
    rng = np.random.default_rng(7)
    for n, m, k, xpad, ypad in [(4099, 17, 33, 3, 0), (2000, 64, 16, 0, 5), (777, 3, 31, 1, 2), (65, 15, 1, 0, 0),
                                (300, 64, 64, 2, 1)]:
        X, Y = _ints(rng, n, m), _ints(rng, n, k)
        got = _gram_raw(hp, X.astype(np.float64), Y.astype(np.float64), xl, yl, xpad, ypad)
        assert np.array_equal(got, (X.T @ Y).astype(np.float64)), (xl, yl, n, m, k)
    # the symmetric path in this layout (X and Y the same buffer)
    X = _ints(rng, 3001, 33)
    got = _gram_raw(hp, X.astype(np.float64), X.astype(np.float64), xl, xl, 1, 1, same=True)
    assert np.array_equal(got, (X.T @ X).astype(np.float64))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 3_000_001])
def test_integer_blocks_bit_equal_every_row_count(hp, n):
    rng = np.random.default_rng(n)
    shapes = [(16, 16), (17, 3)] if n > 100_000 else [(16, 16), (17, 3), (1, 64), (64, 33)]
    for m, k in shapes:
        X, Y = _ints(rng, n, m), _ints(rng, n, k)
        want = (X.T @ Y).astype(np.float64)
        got = _gram_raw(hp, X.astype(np.float64), Y.astype(np.float64))
        assert np.array_equal(got, want), (n, m, k)
        if m == k:
            got = _gram_raw(hp, X.astype(np.float64), X.astype(np.float64), same=True)
            assert np.array_equal(got, (X.T @ X).astype(np.float64)), (n, m)


def test_random_blocks_bound_repeatability_symmetry(hp):
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    rng = np.random.default_rng(3)
    for n, m, k in [(200_003, 16, 16), (50_000, 37, 5), (100_001, 64, 64)]:
        Xg, Yg = rng.uniform(-1, 1, (n, m)), rng.uniform(-1, 1, (n, k))
        X, Y = hp.HPCMatrix.from_global(Xg, backend), hp.HPCMatrix.from_global(Yg, backend)
        C1 = (hp.transpose(X) @ Y).local_values()
        C2 = (hp.transpose(X) @ Y).local_values()
        assert np.array_equal(C1.view(np.uint64), C2.view(np.uint64)), "two calls differ"
        ref = Xg.T @ Yg
        bound = 1e-12 * (np.abs(Xg).T @ np.abs(Yg))
        assert np.all(np.abs(C1 - ref) <= bound), np.max(np.abs(C1 - ref) / bound)
        if m == k:
            S = (hp.transpose(X) @ X).local_values()
            assert np.array_equal(S, S.T), "X'X not exactly symmetric"
            S2 = (hp.transpose(X) @ X).local_values()
            assert np.array_equal(S.view(np.uint64), S2.view(np.uint64))
            assert np.all(np.abs(S - Xg.T @ Xg) <= 1e-12 * (np.abs(Xg).T @ np.abs(Xg)))


def _exact_f32_gram(X32, Y32):
    """float32(exact) of X^T Y: products of floats are exact in double; each entry summed exactly with math.fsum."""
    Xd, Yd = X32.astype(np.float64), Y32.astype(np.float64)
    m, k = Xd.shape[1], Yd.shape[1]
    out = np.empty((m, k), dtype=np.float32)
    for i in range(m):
        P = Xd[:, i:i + 1] * Yd
        for j in range(k):
            out[i, j] = np.float32(math.fsum(P[:, j]))
    return out


def test_float32_within_one_ulp(hp):
    torch = _torch()
    backend = hp.backend_rocm_serial(np.float32, np.int32)
    rng = np.random.default_rng(11)
    for n, m, k in [(40_001, 16, 16), (9_999, 5, 33)]:
        Xg = rng.uniform(-1, 1, (n, m)).astype(np.float32)
        Yg = rng.uniform(-1, 1, (n, k)).astype(np.float32)
        X, Y = hp.HPCMatrix.from_global(Xg, backend), hp.HPCMatrix.from_global(Yg, backend)
        G = hp.transpose(X) @ Y
        assert G.A.dtype == torch.float32
        got = G.local_values()
        want = _exact_f32_gram(Xg, Yg)
        one_ulp = np.spacing(np.abs(want)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= one_ulp), (n, m, k)
        # the raw entry returns double: the same values before the one rounding
        raw = _gram_raw(hp, Xg, Yg, dtype=np.float32)
        assert np.array_equal(raw.astype(np.float32), got)
    Xg = rng.uniform(-1, 1, (12_345, 16)).astype(np.float32)
    X = hp.HPCMatrix.from_global(Xg, backend)
    S = (hp.transpose(X) @ X).local_values()
    assert np.array_equal(S, S.T)


def _spawn(nranks, env_extra):
    from hpcla_amd.launch import spawn_ranks
    return spawn_ranks([WORKER], nranks, env_extra=env_extra, timeout=300, forward_rank0_stdout=False)


@pytest.mark.parametrize("nranks", [2, 3])
def test_gram_across_ranks(nranks):
    """Ranks share the GPU (peer-window all-reduce); one rank has no rows; m is not divisible by the rank count."""
    assert _spawn(nranks, {"HPCLA_PUSH_TIMEOUT_S": "30"}) == 0


@pytest.mark.parametrize("nranks", [2, 3])
def test_gram_across_ranks_mismatched_row_partitions(nranks):
    """Y on another row partition than X: aligned by repartition_dense, whose exchange needs RCCL (one GPU per rank)."""
    if _torch().cuda.device_count() < nranks:
        pytest.skip(f"RCCL needs one GPU per rank ({nranks} ranks)")
    assert _spawn(nranks, {"HPCLA_PUSH_TIMEOUT_S": "30", "HPCLA_GRAM_MISMATCH": "1"}) == 0
