"""The numpy restatement of COO assembly (tests/_assemble_cases.py) against scipy, and the argument rules of
``hp.assembly_plan``, none of which needs a device.

Integer-valued and dyadic values make every order of additions exact, so there the restatement must equal scipy's
``coo_matrix(...).tocsr()`` in every bit.  For random values the two orders differ; each is within the standard bound of a
sum of L terms, |fl(sum) - sum| <= (L - 1) u sum|v| with the unit roundoff u = eps / 2 (to first order), so two sums of the
same terms differ by at most (L - 1) eps sum|v| per entry, eps = 2^-52.  That figure is asserted, and nothing looser."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import _assemble_cases as ac


def _scipy_csr(rows, cols, vals, shape):
    A = sp.coo_matrix((vals, (rows, cols)), shape=shape).tocsr()          # sums duplicates, keeps explicit zeros
    A.sort_indices()
    return A


def _cases():
    out = {}
    out["lengths"] = (ac.planted_lengths(ac.edge_lengths(), (97, 113), 3), (97, 113))
    out["hub"] = ((np.zeros(3000, dtype=np.int64), np.full(3000, 2, dtype=np.int64)), (3, 5))
    out["random"] = (ac.random_coo(20011, (211, 193), 5), (211, 193))
    out["empty_rows"] = ((np.array([2, 3, 7, 3, 2, 7, 7]), np.array([1, 0, 4, 0, 1, 2, 4])), (10, 6))
    return out


@pytest.mark.parametrize("name", list(_cases()))
@pytest.mark.parametrize("kind", ["integer", "dyadic"])
def test_restatement_equals_scipy_exactly(name, kind):
    (rows, cols), shape = _cases()[name]
    vals = ac.values_for(len(rows), 7, kind)
    rowptr, c, v = ac.assemble_ref(rows, cols, vals, shape)
    A = _scipy_csr(rows, cols, vals, shape)
    assert np.array_equal(rowptr, A.indptr) and np.array_equal(c, A.indices)
    got, want = v + 0.0, A.data + 0.0                                     # scipy may start from 0.0: -0.0 + 0.0 = +0.0 on both sides
    assert np.array_equal(ac.bits(got), ac.bits(want))


@pytest.mark.parametrize("name", list(_cases()))
def test_restatement_within_the_summation_bound(name):
    (rows, cols), shape = _cases()[name]
    vals = ac.values_for(len(rows), 9)
    rowptr, c, v = ac.assemble_ref(rows, cols, vals, shape)
    A = _scipy_csr(rows, cols, vals, shape)
    assert np.array_equal(rowptr, A.indptr) and np.array_equal(c, A.indices)
    L = _scipy_csr(rows, cols, np.ones(len(rows)), shape).data
    S = _scipy_csr(rows, cols, np.abs(vals), shape).data
    assert np.all(np.abs(v - A.data) <= (L - 1) * np.finfo(np.float64).eps * S)
    assert L.max() > 2 * ac.CH or name in ("random", "empty_rows")


def test_chunk_rule_is_what_the_text_says():
    """One list of 2 CH + 1 values against two explicit loops."""
    v = ac.values_for(2 * ac.CH + 1, 13)
    parts = []
    for c0 in range(0, len(v), ac.CH):
        s = v[c0]
        for x in v[c0 + 1:c0 + ac.CH]:
            s = s + x
        parts.append(s)
    want = parts[0]
    for p in parts[1:]:
        want = want + p
    got = ac.sum_segments(v, [0, len(v)])
    assert ac.bits(got)[0] == ac.bits(np.array([want]))[0]
    plain = v[0]
    for x in v[1:]:
        plain = plain + x
    assert ac.bits(ac.sum_segments(v, [0, len(v)], ch=10 ** 6))[0] == ac.bits(np.array([plain]))[0]
    assert ac.bits(ac.sum_segments(np.array([-0.0]), [0, 1]))[0] == ac.bits(np.array([-0.0]))[0]      # a lone -0.0 stays
    assert ac.bits(ac.sum_segments(np.array([1.5, -1.5]), [0, 0, 2]))[1] == 0                       # x + (-x) = +0.0
    assert ac.bits(ac.sum_segments(np.array([1.5, -1.5]), [0, 0, 2]))[0] == 0                       # an empty list: +0.0


def test_p1_fixture_is_the_five_point_matrix_plus_identity():
    nx, ny = 33, 31
    rows, cols, vals = ac.p1_triplets(nx, ny)
    rowptr, c, v = ac.assemble_ref(rows, cols, vals, (nx * ny, nx * ny))
    E = ac.p1_expected(nx, ny)
    assert np.array_equal(rowptr, E.indptr) and np.array_equal(c, E.indices)
    assert np.array_equal(ac.bits(v + 0.0), ac.bits(E.data + 0.0))
    p = 5 + nx * 7                                                        # a node inside the grid
    row = dict(zip(c[rowptr[p]:rowptr[p + 1]].tolist(), v[rowptr[p]:rowptr[p + 1]].tolist()))
    assert row == {p - nx: -1.0, p - nx + 1: 0.0, p - 1: -1.0, p: 5.0, p + 1: -1.0, p + nx - 1: 0.0, p + nx: -1.0}
    assert np.count_nonzero(v == 0.0) == 2 * (nx - 1) * (ny - 1)          # the cells' diagonals are stored, as explicit zeros
    S = _scipy_csr(rows, cols, vals, (nx * ny, nx * ny))
    assert np.array_equal(S.indices, c) and np.array_equal(ac.bits(S.data + 0.0), ac.bits(v + 0.0))


def test_vector_restatement():
    idx = np.array([9, 0, 4, 9, 0, 0])
    vals = np.array([1.0, 2.0, -0.0, 0.25, 4.0, 8.0])
    got = ac.assemble_vector_ref(idx, vals, 10)
    want = np.zeros(10)
    want[[0, 4, 9]] = [14.0, -0.0, 1.25]
    assert np.array_equal(ac.bits(got), ac.bits(want))
    own = idx >= 4                                                        # the slice [4, 10) of a rank that owns it
    assert np.array_equal(ac.bits(ac.assemble_vector_ref(idx[own], vals[own], 10, 4, 10)), ac.bits(want[4:]))


# -- argument rules: nothing here touches a device ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_backend(hp):
    return hp.HPCBackend(np.float64, np.int32, hp.DeviceCPU(), hp.CommSerial(), hp.SolverNone())


def test_argument_rules_raise_without_a_device(hp, cpu_backend):
    r, c = np.array([0, 1, 2]), np.array([2, 1, 0])
    with pytest.raises(ValueError, match="differ in length"):
        hp.assembly_plan(r, c[:2], (3, 3), cpu_backend)
    with pytest.raises(TypeError, match="integers"):
        hp.assembly_plan(r.astype(np.float64), c, (3, 3), cpu_backend)
    with pytest.raises(TypeError, match="int64"):
        import torch
        hp.assembly_plan(torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), (3, 3), cpu_backend)
    with pytest.raises(IndexError, match=r"2 of the indices .*first is \(-1, 1\) at position 1"):
        hp.assembly_plan(np.array([0, -1, 2, 1]), np.array([2, 1, 3, 1]), (3, 3), cpu_backend)
    with pytest.raises(IndexError, match="row 7 at position 0"):
        hp.assembly_plan(np.array([7]), None, (7,), cpu_backend)
    with pytest.raises(ValueError, match="63-bit key"):
        hp.assembly_plan(np.array([0]), np.array([0]), (2 ** 40, 2 ** 30), cpu_backend)
    with pytest.raises(ValueError, match="shape"):
        hp.assembly_plan(r, c, (3,), cpu_backend)
    with pytest.raises(ValueError, match="shape"):
        hp.assembly_plan(r, None, (3, 3), cpu_backend)
    with pytest.raises(ValueError, match="one-dimensional"):
        hp.assembly_plan(np.zeros((2, 2), dtype=np.int64), np.zeros((2, 2), dtype=np.int64), (3, 3), cpu_backend)
    with pytest.raises(ValueError, match="row_partition"):
        hp.assembly_plan(r, c, (3, 3), cpu_backend, row_partition=[0, 2])
    f32 = hp.HPCBackend(np.float32, np.int32, hp.DeviceCPU(), hp.CommSerial(), hp.SolverNone())
    with pytest.raises(TypeError, match="Float64 backends only"):
        hp.assembly_plan(r, c, (3, 3), f32)
    with pytest.raises(TypeError, match="no CPU compute path"):           # the arguments pass; there is no host fallback
        hp.assembly_plan(r, c, (3, 3), cpu_backend)


def test_value_rules_raise_without_a_device(hp):
    from hpcla_amd import assemble as asm
    with pytest.raises(ValueError, match="3 values"):
        asm.check_values(np.zeros(4), 3)
    with pytest.raises(TypeError, match="float64"):
        asm.check_values(np.zeros(3, dtype=np.float32), 3)
    with pytest.raises(ValueError, match="3 values"):
        asm.check_values(np.zeros((3, 1)), 3)
    with pytest.raises(TypeError, match="float64"):
        hp.sparse_from_coo(np.array([0]), np.array([0]), np.array([1], dtype=np.int64), (1, 1), None)
    assert asm.check_values(np.zeros(3), 3).shape == (3,)
