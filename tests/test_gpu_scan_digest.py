"""GPU tests of the device-wide scan past its first trip of block sums and of the structure digest against its host twin.

The scan (csrc/scan.h) sums blocks of 1024 elements and one workgroup then scans those block sums 256 at a time, carrying the
running total from trip to trip: the carry first matters for a scan of more than 256 * 1024 = 262 144 elements.  The column-space
construction scans a presence bitmap of its window, so its windows here are 262 144 (256 blocks, one trip), 262 145 (257 blocks: the
second trip has one live lane) and 614 403 (601 blocks: a ragged third trip); tests/test_grid_regimes.py checks these counts.  The
ids are a seeded random subset of the window whose density changes by region, with empty regions, so block sums differ and a carry
taken from the wrong trip cannot come out right.  Reference: numpy's unique and searchsorted; everything is compared exactly.

The digest (csrc/construct.hip) is a grid-stride loop of at most 4096 * 256 lanes, so element 1 048 576 is the first of a second
pass.  ``partition.array_digest`` states the same formula in numpy; the two must give the same 32 bytes, or a device-built and a
host-built matrix of one structure would not share a cached plan -- and a digest that misses elements would let two structures
share one."""
import ctypes

import numpy as np
import pytest

from tests import _grid_regimes as gr

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- the scan ----------------------------------------------------------------------------------------------------------------
def _window_ids(width, col_lo):
    """Global column ids of at most 200 000 nonzeros in [col_lo, col_lo + width): regions of 8192 ids (8 scan blocks) with
    densities from none to 0.7, the first and last id of the window and the ids on either side of the first carry; in shuffled
    order, a tenth of them twice."""
    rng = np.random.default_rng(width)
    picks = [np.array([0, width - 1, gr.SCAN_CARRY_AT - 1, min(gr.SCAN_CARRY_AT, width - 1)], dtype=np.int64)]
    for lo in range(0, width, 8192):
        hi = min(lo + 8192, width)
        density = rng.choice([0.0, 0.0, 0.002, 0.02, 0.2, 0.7])
        picks.append(lo + np.flatnonzero(rng.random(hi - lo) < density))
    uniq = np.unique(np.concatenate(picks))
    ids = np.concatenate([uniq, rng.choice(uniq, size=len(uniq) // 10)])
    rng.shuffle(ids)
    assert len(ids) <= 200_000
    return ids + col_lo


@pytest.mark.parametrize("sfx", ["i32", "i64"])
@pytest.mark.parametrize("width,col_lo", gr.SCAN_WINDOWS)
def test_compress_columns_carries_across_trips_of_block_sums(hp, width, col_lo, sfx):
    import torch
    lib = hp._capi.load()
    ids = _window_ids(width, col_lo)
    want_ci, want_cv = np.unique(ids), None
    want_cv = np.searchsorted(want_ci, ids)
    sums = np.add.reduceat(np.isin(np.arange(col_lo, col_lo + width), want_ci).astype(np.int64), np.arange(0, width, gr.SCAN_B))
    assert len(sums) == gr.scan_blocks(width) and (sums == 0).any() and len(np.unique(sums)) > 20
    if gr.scan_trips(width) > 1:
        assert sums[:gr.SCAN_T].sum() != sums[gr.SCAN_T:2 * gr.SCAN_T].sum()           # the trips' totals differ
    ids_d = _t(ids)
    work = torch.empty(lib.hpcla_colspace_work_bytes(width), dtype=torch.uint8, device="cuda")
    tdt, ndt = (torch.int32, np.int32) if sfx == "i32" else (torch.int64, np.int64)
    for base in (0, 1):
        cv = torch.full((len(ids),), -7, dtype=tdt, device="cuda")
        ci = torch.full((width,), -7, dtype=torch.int64, device="cuda")
        ncomp = ctypes.c_int64(-1)
        hp._capi.call(f"hpcla_compress_columns_{sfx}", ids_d.data_ptr(), len(ids), col_lo, width, cv.data_ptr(), base,
                      ci.data_ptr(), ctypes.byref(ncomp), work.data_ptr(), _stream())
        assert ncomp.value == len(want_ci)
        np.testing.assert_array_equal(ci[:ncomp.value].cpu().numpy(), want_ci)
        np.testing.assert_array_equal(cv.cpu().numpy(), (want_cv + base).astype(ndt))
        assert bool((ci[ncomp.value:] == -7).all())                                     # nothing is written past the count


def test_device_built_matrix_over_a_window_of_several_trips(hp, orc, gpu_backend_i32):
    """The same through HPCSparseMatrix_local_device, with orc.compress_columns as the reference: one entry per row at the ids of
    the 601-block window, so the product gathers x through the compressed columns."""
    width, col_lo = gr.SCAN_WINDOWS[2]
    ids = _window_ids(width, col_lo)
    n, ncols = len(ids), col_lo + width + 5
    rowptr = np.arange(n + 1, dtype=np.int64)
    vals = np.random.default_rng(5).standard_normal(n)
    rows = orc.LocalRows(rowptr, ids, vals, ncols)
    ci_ref, cv_ref = orc.compress_columns(rows)
    A = hp.HPCSparseMatrix_local_device(_t(rowptr), _t(ids), _t(vals), ncols, gpu_backend_i32,
                                        col_window=(col_lo, col_lo + width - 1))
    np.testing.assert_array_equal(A.col_indices, ci_ref)
    np.testing.assert_array_equal(A.colval, cv_ref)
    assert A.ncols_compressed == len(ci_ref)


# ---- the digest --------------------------------------------------------------------------------------------------------------
def _digest(hp, a):
    out = (ctypes.c_uint64 * 4)()
    sfx = "i32" if a.dtype == np.int32 else "i64"
    d = _t(a) if a.size else None
    hp._capi.call(f"hpcla_digest_{sfx}", d.data_ptr() if a.size else None, a.size, out, _stream())
    return bytes(out)


@pytest.mark.parametrize("n", gr.DIGEST_SIZES)
def test_device_digest_equals_its_host_twin(hp, n):
    """n = 1, 255, 257: one lane, a workgroup short of full, two workgroups; 1 048 576 = 4096 * 256 fills the capped grid in one
    pass, 1 048 577 leaves one element to a second pass and 2 500 003 ends in a ragged third pass.  Both widths; 64-bit values
    are negative and beyond 2^31 as well."""
    from hpcla_amd.partition import array_digest
    rng = np.random.default_rng(n)
    a32 = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    a64 = rng.integers(-2**40, 2**40, n, dtype=np.int64)
    a64[0], a64[-1] = -(2**33) - 5, 2**31 + 7
    base32, base64 = _digest(hp, a32), _digest(hp, a64)
    assert base32 == array_digest(a32) and base64 == array_digest(a64)
    assert base32 == _digest(hp, a32.astype(np.int64)) == array_digest(a32.astype(np.int64))     # the width does not enter
    assert len(set(base64[8 * k:8 * k + 8] for k in range(4))) == 4 and base32 != base64
    for a, base in ((a32, base32), (a64, base64)):
        changed = [n - 1] + ([gr.DIGEST_CAP * gr.DIGEST_T] if n > gr.DIGEST_CAP * gr.DIGEST_T else [])
        for at in changed:                                   # the last element; the first element of the second pass
            b = a.copy()
            b[at] ^= 1
            got = _digest(hp, b)
            assert got != base and got == array_digest(b), at
        if n >= 2:                                           # the position enters: two unequal elements swapped
            i, j = 0, n - 1
            assert a[i] != a[j]
            b = a.copy()
            b[i], b[j] = a[j], a[i]
            got = _digest(hp, b)
            assert got != base and got == array_digest(b)


def test_digest_of_nothing_is_four_zero_words(hp):
    from hpcla_amd.partition import array_digest
    for dt in (np.int32, np.int64):
        assert _digest(hp, np.empty(0, dtype=dt)) == bytes(32) == array_digest(np.empty(0, dtype=dt))
