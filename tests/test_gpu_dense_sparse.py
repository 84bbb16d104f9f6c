"""Dense times sparse on the GPU: transpose(X) * A and X * A (csrc/spmm_t.hip, dense.dense_sparse_matmat[_t]) and
transpose(X).materialize().

* the reference's own fixture (test/test_new_operations.jl:91-120: E (6 x 8) * D (8 x 6), transpose(B) * A_sparse)
  through the public operators, against numpy, with the reference's result partitions;
* integer-valued X and A (every partial sum exact): bit-equal to numpy's int64 product for widths 1 .. 64, row- and
  column-major X with padded leading dimensions (and the odd-width padded-pitch block an SpMM returns), Int32 and Int64
  indices (narrowed and not), a non-square A with empty rows and empty columns;
* bit identity with the existing paths at N = 1: transpose(X) * A == (transpose(A) * X)^T and
  X * A == transpose(transpose(A) * transpose(X).materialize()) for a non-symmetric A;
* random inputs: |C - C_exact| <= 1e-12 |X|^T |A| componentwise, identical bits on a second call, and 2 * A (shared
  structure, new values) doubles the result exactly;
* the config-2 matrix (4096^2 5-point Poisson) with m = 16: transpose(X) * A == (A * X)^T bit for bit (A is symmetric);
* several ranks (tests/_multirank_dense_sparse_worker.py): the reverse exchange needs RCCL, one GPU per rank.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_multirank_dense_sparse_worker.py")

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 15, 16, 17, 33, 64)


def _torch():
    import torch
    return torch


def _dense(hp, backend, M, layout="row", pad=0):
    """HPCMatrix holding the global (1-rank) block M in the given device layout, `pad` spare entries per stride."""
    torch = _torch()
    n, w = M.shape
    if layout == "row":
        buf = torch.full((n, w + pad), 7.0, dtype=torch.float64, device="cuda")
        buf[:, :w] = torch.from_numpy(np.ascontiguousarray(M))
        T = buf[:, :w]
    else:
        buf = torch.full((w, n + pad), 7.0, dtype=torch.float64, device="cuda")
        buf[:, :n] = torch.from_numpy(np.ascontiguousarray(M.T))
        T = buf[:, :n].t()
    return hp.HPCMatrix(hp.uniform_partition(n, 1), hp.uniform_partition(w, 1), T, backend)


def _int_sparse(rng, p, n, density=0.05, empty_rows=(), empty_cols=()):
    S = sp.random(p, n, density=density, format="csr", random_state=np.random.RandomState(int(rng.integers(1 << 30))),
                  data_rvs=lambda k: rng.integers(-9, 10, size=k).astype(np.float64))
    S = S.tolil()
    for r in empty_rows:
        S[r, :] = 0
    for c in empty_cols:
        S[:, c] = 0
    S = S.tocsr()
    S.eliminate_zeros()
    return S


def _exact(Xi, S):
    return (Xi.astype(np.int64) @ S.toarray().astype(np.int64)).astype(np.float64)


def test_reference_fixture_through_the_operators(hp):
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    n, m = 8, 6
    I = np.arange(8)
    A0 = sp.csr_matrix((np.array([1, 2, 3, 4, 5, 6, 7, 8, .1, .2, .3, .4, .5, .6, .7, .8]),
                        (np.concatenate([I, I]), np.concatenate([I, (I + 1) % 8]))), shape=(n, n))
    Ag = (A0 + A0.T + 2 * sp.identity(n)).tocsr()
    Bg = np.array([[i + j * 0.1 for j in range(1, m + 1)] for i in range(1, n + 1)])
    Dg = sp.csr_matrix((np.arange(1.0, 7.0), (np.arange(6), np.arange(6))), shape=(n, m))
    Eg = np.array([[i * 0.2 + j * 0.3 for j in range(1, n + 1)] for i in range(1, m + 1)])
    A = hp.HPCSparseMatrix_from_global(Ag, backend)
    D = hp.HPCSparseMatrix_from_global(Dg, backend)
    B = hp.HPCMatrix.from_global(Bg, backend)
    E = hp.HPCMatrix.from_global(Eg, backend)
    R4 = E * D                                               # HPCMatrix * HPCSparseMatrix
    R6 = hp.transpose(B) @ A                                 # transpose(HPCMatrix) * HPCSparseMatrix
    assert isinstance(R4, hp.HPCMatrix) and isinstance(R6, hp.HPCMatrix)
    np.testing.assert_allclose(R4.gather(), Eg @ Dg.toarray(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R6.gather(), Bg.T @ Ag.toarray(), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(R4.row_partition, E.row_partition)
    np.testing.assert_array_equal(R4.col_partition, hp.uniform_partition(m, 1))
    np.testing.assert_array_equal(R6.row_partition, B.col_partition)
    np.testing.assert_array_equal(R6.col_partition, hp.uniform_partition(n, 1))
    Bt = hp.transpose(B).materialize()
    np.testing.assert_array_equal(Bt.gather(), Bg.T)
    np.testing.assert_array_equal(Bt.row_partition, B.col_partition)
    np.testing.assert_array_equal(Bt.col_partition, B.row_partition)
    with pytest.raises(ValueError):
        hp.transpose(E) @ A                                  # E has 6 rows, A 8
    with pytest.raises(ValueError):
        B @ A                                                # B has 6 columns, A 8 rows


@pytest.mark.parametrize("m", WIDTHS)
def test_integer_inputs_bit_equal_every_width(hp, m):
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    rng = np.random.default_rng(100 + m)
    p, n = 1001, 777                                         # non-square, empty rows and columns
    S = _int_sparse(rng, p, n, empty_rows=(0, 5, 500, p - 1), empty_cols=(0, 3, 400, n - 1))
    A = hp.HPCSparseMatrix_from_global(S, backend)
    Xg = rng.integers(-8, 9, size=(p, m)).astype(np.float64)
    Zg = rng.integers(-8, 9, size=(m, p)).astype(np.float64)
    got = (hp.transpose(_dense(hp, backend, Xg)) @ A).gather()
    assert got.shape == (m, n)
    np.testing.assert_array_equal(got, _exact(Xg.T, S))
    got = (_dense(hp, backend, Zg) @ A).gather()
    assert got.shape == (m, n)
    np.testing.assert_array_equal(got, _exact(Zg, S))


@pytest.mark.parametrize("layout,pad", [("row", 0), ("row", 3), ("col", 0), ("col", 5)])
@pytest.mark.parametrize("index", ["i32", "i64", "i64-wide"])
def test_integer_inputs_bit_equal_every_layout_and_index_type(hp, monkeypatch, layout, pad, index):
    if index == "i64-wide":
        monkeypatch.setenv("HPCLA_NARROW_INDICES", "0")      # an Int64 plan on the Int64 kernels
    backend = hp.backend_rocm_serial(np.float64, np.int32 if index == "i32" else np.int64)
    rng = np.random.default_rng(7)
    p, n = 2345, 1999
    S = _int_sparse(rng, p, n, density=0.01, empty_rows=(1, 2, 3), empty_cols=(10, 11))
    A = hp.HPCSparseMatrix_from_global(S, backend)
    for m in (3, 16, 17):
        Xg = rng.integers(-8, 9, size=(p, m)).astype(np.float64)
        Zg = rng.integers(-8, 9, size=(m, p)).astype(np.float64)
        np.testing.assert_array_equal((hp.transpose(_dense(hp, backend, Xg, layout, pad)) @ A).gather(), _exact(Xg.T, S))
        np.testing.assert_array_equal((_dense(hp, backend, Zg, layout, pad) @ A).gather(), _exact(Zg, S))
    if index == "i64-wide":
        assert hp.dense._spmm_t_plan(A).is_i64
    elif index == "i64":
        assert not hp.dense._spmm_t_plan(A).is_i64       # narrowed, as the SpMV plans are


def test_integer_inputs_padded_pitch_block_of_an_spmm(hp):
    """X = A1 * B with an odd width: the (rows, k) view of a (rows, k + 1) buffer (spmm_plans.spmm_pitch)."""
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    rng = np.random.default_rng(3)
    p, n, k = 1500, 900, 15
    S1 = _int_sparse(rng, p, p, density=0.002)
    S = _int_sparse(rng, p, n, density=0.01)
    Bg = rng.integers(-2, 3, size=(p, k)).astype(np.float64)
    X = hp.HPCSparseMatrix_from_global(S1, backend) @ hp.HPCMatrix.from_global(Bg, backend)
    assert X.A.stride(0) == k + 1                            # the padded pitch this test is about
    Xg = (S1.toarray().astype(np.int64) @ Bg.astype(np.int64)).astype(np.float64)
    np.testing.assert_array_equal(X.gather(), Xg)
    A = hp.HPCSparseMatrix_from_global(S, backend)
    np.testing.assert_array_equal((hp.transpose(X) @ A).gather(), _exact(Xg.T, S))
    Xt = hp.transpose(X).materialize()                       # k x p: X^T materialised, then X * A on it
    np.testing.assert_array_equal(Xt.gather(), Xg.T)
    np.testing.assert_array_equal((Xt @ A).gather(), _exact(Xg.T, S))


@pytest.mark.parametrize("index", ["i32", "i64-wide"])
def test_row_major_W_and_strided_X_through_the_c_abi(hp, monkeypatch, index):
    """The layouts the one-rank Python path does not take: W row-major (every N > 1 call, every Julia call) with a padded
    leading dimension, odd and even m, and a column-major X read in place -- the padding of W left untouched."""
    torch = _torch()
    from hpcla_amd.vectors import current_stream_ptr, dptr
    if index == "i64-wide":
        monkeypatch.setenv("HPCLA_NARROW_INDICES", "0")
    backend = hp.backend_rocm_serial(np.float64, np.int32 if index == "i32" else np.int64)
    rng = np.random.default_rng(31)
    p, n = 1777, 1301
    S = _int_sparse(rng, p, n, density=0.01, empty_rows=(0, 9), empty_cols=(2, n - 1))
    A = hp.HPCSparseMatrix_from_global(S, backend)
    plan = hp.dense._spmm_t_plan(A)
    assert plan.host.ncols_split == n and plan.is_i64 == (index == "i64-wide")
    sfx = "i64" if plan.is_i64 else "i32"
    lib = hp._capi
    for m in (1, 2, 3, 16, 17):
        Xg = rng.integers(-8, 9, size=(p, m)).astype(np.float64)
        want = _exact(Xg.T, S).T                                  # n x m
        for x_layout in ("row", "col"):
            Xm = _dense(hp, backend, Xg, x_layout, pad=2)
            ldx = int(Xm.A.stride(0) if x_layout == "row" else Xm.A.stride(1))
            for pad in (0, 3):
                ldw = m + pad
                W = torch.full((n, ldw), 7.0, dtype=torch.float64, device="cuda")
                lib.call(f"hpcla_spmm_t_f64_{sfx}", dptr(plan.colptr), dptr(plan.rowidx), dptr(plan.perm), dptr(A.nzval), n,
                         dptr(Xm.A), ldx, lib.LAYOUT_ROW if x_layout == "row" else lib.LAYOUT_COL, m, dptr(W), ldw,
                         lib.LAYOUT_ROW, current_stream_ptr())
                got = W.cpu().numpy()
                np.testing.assert_array_equal(got[:, :m], want, err_msg=f"m={m} x={x_layout} pad={pad}")
                assert np.all(got[:, m:] == 7.0)


def test_accumulate_kernel_against_numpy(hp):
    """hpcla_spmm_t_accumulate_f64 on hand-built lists: own rows plus received rows, in list order, padded strides."""
    torch = _torch()
    from hpcla_amd.vectors import current_stream_ptr, dptr
    rng = np.random.default_rng(5)
    for m in (1, 3, 16, 33):
        ldv, ldr = m + 2, m + 1
        V0 = rng.uniform(-1, 1, (50, ldv))
        R = rng.uniform(-1, 1, (40, ldr))
        rows = np.array([0, 3, 7, 49], dtype=np.int64)
        ptr = np.array([0, 1, 4, 4, 9], dtype=np.int64)          # one row with nothing to add
        pos = np.array([5, 0, 39, 5, 1, 2, 3, 4, 10], dtype=np.int64)
        want = V0.copy()
        for u, r in enumerate(rows):
            acc = want[r, :m].copy()
            for t in range(ptr[u], ptr[u + 1]):
                acc = acc + R[pos[t], :m]
            want[r, :m] = acc
        Vd = torch.from_numpy(V0.copy()).cuda()
        Rd = torch.from_numpy(R).cuda()
        up = lambda a: torch.from_numpy(a).cuda()
        rows_d, ptr_d, pos_d = up(rows), up(ptr), up(pos)
        hp._capi.call("hpcla_spmm_t_accumulate_f64", dptr(Vd), ldv, dptr(Rd), ldr, dptr(rows_d), dptr(ptr_d), dptr(pos_d),
                      len(rows), m, current_stream_ptr())
        assert np.array_equal(Vd.cpu().numpy(), want), m


def test_bit_identity_with_the_existing_paths(hp):
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    rng = np.random.default_rng(11)
    p, n, m = 3000, 2500, 16
    S = sp.random(p, n, density=0.004, format="csr", random_state=np.random.RandomState(5))
    S.data = rng.uniform(-1, 1, S.nnz)
    A = hp.HPCSparseMatrix_from_global(S, backend)
    X = hp.HPCMatrix.from_global(rng.uniform(-1, 1, (p, m)), backend)
    left = (hp.transpose(X) @ A).gather()
    right = (hp.transpose(A) @ X).gather().T                 # the materialised A^T, then the tuned SpMM
    assert np.array_equal(left, right)
    Z = hp.HPCMatrix.from_global(rng.uniform(-1, 1, (m, p)), backend)
    got = (Z @ A).gather()
    want = (hp.transpose(A) @ hp.transpose(Z).materialize()).gather().T
    assert np.array_equal(got, want)


def test_random_bound_repeatability_and_new_values(hp):
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    rng = np.random.default_rng(21)
    p, n, m = 5000, 4000, 17
    S = sp.random(p, n, density=0.003, format="csr", random_state=np.random.RandomState(8))
    S.data = rng.uniform(-1, 1, S.nnz)
    A = hp.HPCSparseMatrix_from_global(S, backend)
    Xg = rng.uniform(-1, 1, (p, m))
    X = hp.HPCMatrix.from_global(Xg, backend)
    C1 = (hp.transpose(X) @ A).gather()
    exact = Xg.T @ S.toarray()
    bound = 1e-12 * (np.abs(Xg).T @ np.abs(S.toarray()))
    assert np.all(np.abs(C1 - exact) <= bound)
    C2 = (hp.transpose(X) @ A).gather()
    assert np.array_equal(C1, C2)
    A2 = 2 * A                                               # shared structure, new values
    assert A2.structural_hash == A.structural_hash
    assert np.array_equal((hp.transpose(X) @ A2).gather(), 2 * C1)
    Z = hp.HPCMatrix.from_global(Xg.T.copy(), backend)
    D1 = (Z @ A).gather()
    assert np.all(np.abs(D1 - exact) <= bound)
    assert np.array_equal((Z @ A2).gather(), 2 * D1)


def test_float32_backends_keep_raising(hp):
    backend = hp.backend_rocm_serial(np.float32, np.int32)
    S = sp.random(40, 30, density=0.1, format="csr", random_state=np.random.RandomState(1))
    A = hp.HPCSparseMatrix_from_global(S, backend)
    with pytest.raises(TypeError):
        hp.transpose(hp.HPCMatrix.from_global(np.ones((40, 4)), backend)) @ A
    with pytest.raises(TypeError):
        hp.HPCMatrix.from_global(np.ones((4, 40)), backend) @ A


def test_config2_full_size_matches_the_spmm(hp, orc, gpu_backend_i32):
    """The 4096^2 5-point matrix (symmetric) with m = 16: transpose(X) * A == (A * X)^T bit for bit."""
    torch = _torch()
    N = 4096
    n = N * N
    s0 = torch.cuda.current_stream().cuda_stream
    nnz = hp._capi.load().hpcla_poisson2d_nnz(N, N, 0, n)
    rp_d = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ci_d = torch.empty(nnz, dtype=torch.int64, device="cuda")
    va_d = torch.empty(nnz, dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_gen_poisson2d", N, N, 0, n, rp_d.data_ptr(), ci_d.data_ptr(), va_d.data_ptr(), s0)
    A = hp.HPCSparseMatrix_local_device(rp_d, ci_d, va_d, n, gpu_backend_i32, col_window=(0, n - 1))
    del ci_d, rp_d
    Xl = torch.empty((n, 16), dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_fill_uniform_f64", Xl.data_ptr(), 0, n * 16, orc.SEED_X, s0)
    X = hp.HPCMatrix_local(Xl, gpu_backend_i32)
    C = hp.transpose(X) @ A
    Y = A @ X
    assert tuple(C.A.shape) == (16, n)
    assert torch.equal(C.A, Y.A.t())
    C2 = hp.transpose(X) @ A
    assert torch.equal(C.A, C2.A)
    del A, X, Xl, C, C2, Y, va_d
    hp.clear_spmm_cache()
    hp.clear_plan_cache()
    torch.cuda.empty_cache()


def _spawn(nranks, env_extra):
    from hpcla_amd.launch import spawn_ranks
    return spawn_ranks([WORKER], nranks, env_extra=env_extra, timeout=300, forward_rank0_stdout=False)


@pytest.mark.parametrize("nranks", [2, 3])
def test_dense_sparse_across_ranks(nranks):
    """One rank without rows, m not divisible by the rank count; the reverse exchange goes through RCCL."""
    if _torch().cuda.device_count() < nranks:
        pytest.skip(f"RCCL needs one GPU per rank ({nranks} ranks)")
    assert _spawn(nranks, {"HPCLA_PUSH_TIMEOUT_S": "30"}) == 0
