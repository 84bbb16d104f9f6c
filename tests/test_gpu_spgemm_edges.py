"""The SpGEMM kernels of csrc/spgemm.hip where they branch: rows on, one below and one above every bin cap, every row
through every bin that admits it, partial workgroups, column ids at the 2^58 limit, the upper-bound and compaction kernels,
and product lists whose entries start, end and continue across the streaming kernel's 1024-product passes -- through the raw
C ABI (both index types, both index bases, both list-pointer widths), plus the host layer at its row limit.

Every comparison is bit for bit against tests/_spgemm_edge_cases.py (gustavson_ref / mapped_ref, proved equal to the C
oracle on the CPU in tests/test_spgemm_edge_cases.py).  Outputs start as sentinels (NaN values, -1 columns and counts), so
a slot the kernel must not write is seen when it does.

A row is NEVER given to a bin whose cap is below its upper bound: the hash tables are sized for the cap, find-or-insert in a
full table never terminates, and a hung kernel on a shared machine is not a test result."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _spgemm_edge_cases import (ROW_FAMILIES, bin_rows, gustavson_ref, mapped_case, mapped_lists, mapped_ref,  # noqa: E402
                                order_sensitive, ub_case)

pytestmark = pytest.mark.gpu

ROWS_PER_WORKGROUP = (16, 8, 4, 4, 1)     # numeric_launch in csrc/spgemm.hip, bins 0..4
GAP = 3                                   # sentinel slots between the rows' upper-bound regions
NAN_BITS = np.array([np.nan]).view(np.uint64)[0]


@pytest.fixture(scope="module")
def caps(hp):
    lib = hp._capi.load()
    out = []
    while lib.hpcla_spgemm_bin_cap(len(out)) >= 0:
        out.append(int(lib.hpcla_spgemm_bin_cap(len(out))))
    assert len(out) == len(ROWS_PER_WORKGROUP) and lib.hpcla_spgemm_bin_cap(-1) == -1
    return tuple(out)


_family_cache = {}


def _family(name, caps):
    """(case, reference), computed once per session and never written to."""
    if name not in _family_cache:
        c = ROW_FAMILIES[name](caps)
        _family_cache[name] = (c, gustavson_ref(c["a_rowptr"], c["a_col"], c["a_val"], c["g_rowptr"], c["g_col"], c["g_val"]))
    return _family_cache[name]


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _DeviceCase:
    """A case's arrays on the device in the index type and base of one raw-ABI call."""

    def __init__(self, c, which, base):
        Ti = np.int32 if which == "i32" else np.int64
        self.sfx, self.base = which, base
        self.a_rowptr, self.a_col = _dev((c["a_rowptr"] + base).astype(Ti)), _dev((c["a_col"] + base).astype(Ti))
        self.a_val = _dev(c["a_val"])
        self.g_rowptr, self.g_col, self.g_val = _dev(c["g_rowptr"]), _dev(c["g_col"]), _dev(c["g_val"])


def _slots(ub, order):
    """Upper-bound regions laid out in `order` (a permutation of the rows) with GAP sentinel slots after each; returns
    (ub_prefix per row, total)."""
    ub_prefix = np.zeros(len(ub), dtype=np.int64)
    off = 0
    for r in order:
        ub_prefix[r] = off
        off += int(ub[r]) + GAP
    return ub_prefix, off


def _run_numeric_and_check(hp, d, c, ref, b, row_list, ub_prefix, total, what):
    """One hpcla_spgemm_numeric_* call for bin b over `row_list`; asserts counts, columns and values bit for bit and that
    everything the call must not write still holds its sentinel."""
    import torch
    nrows = len(c["ub"])
    ref_rp, ref_col, ref_val = ref
    row_list = np.asarray(row_list, dtype=np.int32)
    d_list = _dev(row_list) if len(row_list) else None
    d_prefix = _dev(ub_prefix)
    col_tmp = torch.full((total,), -1, dtype=torch.int64, device="cuda")
    val_tmp = torch.full((total,), float("nan"), dtype=torch.float64, device="cuda")
    cnt = torch.full((nrows,), -1, dtype=torch.int64, device="cuda")
    hp._capi.call(f"hpcla_spgemm_numeric_{d.sfx}", b, d.a_rowptr.data_ptr(), d.a_col.data_ptr(), d.a_val.data_ptr(), d.base,
                  d.g_rowptr.data_ptr(), d.g_col.data_ptr(), d.g_val.data_ptr(),
                  d_list.data_ptr() if d_list is not None else None, len(row_list), d_prefix.data_ptr(),
                  col_tmp.data_ptr(), val_tmp.data_ptr(), cnt.data_ptr(), _stream())
    torch.cuda.synchronize()
    got_col, got_bits, got_cnt = col_tmp.cpu().numpy(), val_tmp.cpu().numpy().view(np.uint64), cnt.cpu().numpy()
    want_col = np.full(total, -1, dtype=np.int64)
    want_bits = np.full(total, NAN_BITS, dtype=np.uint64)
    want_cnt = np.full(nrows, -1, dtype=np.int64)
    specified = np.ones(total, dtype=bool)             # slots cnt[i] .. ub[i] of a listed row are the kernel's to leave or use
    for r in row_list.tolist():
        n, off = int(ref_rp[r + 1] - ref_rp[r]), int(ub_prefix[r])
        want_cnt[r] = n
        want_col[off:off + n] = ref_col[ref_rp[r]:ref_rp[r + 1]]
        want_bits[off:off + n] = ref_val[ref_rp[r]:ref_rp[r + 1]].view(np.uint64)
        specified[off + n:off + int(c["ub"][r])] = False
    np.testing.assert_array_equal(got_cnt, want_cnt, err_msg=f"{what}: cnt")
    for r in row_list.tolist():                          # row by row first: a failure then names the row and its ub
        n, off = int(want_cnt[r]), int(ub_prefix[r])
        np.testing.assert_array_equal(got_col[off:off + n], want_col[off:off + n],
                                      err_msg=f"{what}: columns of row {r} (ub {int(c['ub'][r])})")
        np.testing.assert_array_equal(got_bits[off:off + n], want_bits[off:off + n],
                                      err_msg=f"{what}: value bits of row {r} (ub {int(c['ub'][r])})")
    np.testing.assert_array_equal(got_col[specified], want_col[specified], err_msg=f"{what}: a column slot outside the listed rows")
    np.testing.assert_array_equal(got_bits[specified], want_bits[specified], err_msg=f"{what}: a value slot outside the listed rows")


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("which", ["i32", "i64"])
def test_ub_kernel(hp, which, base):
    """hpcla_spgemm_ub_* against numpy at 1, 255, 256 and 257 rows (one thread per row, 256 per workgroup), empty rows among
    them, and a sum past int32: three referenced G rows of 2^30 entries each (the kernel reads only g_rowptr)."""
    import torch
    Ti = np.int32 if which == "i32" else np.int64
    cases = [ub_case(n, n) for n in (1, 255, 256, 257)]
    cases.append((np.array([0, 0, 3, 4], dtype=np.int64), np.array([0, 1, 2, 1], dtype=np.int64),
                  np.array([0, 2 ** 30, 2 ** 31, 3 * 2 ** 30], dtype=np.int64)))
    for a_rowptr, a_col, g_rowptr in cases:
        nrows = len(a_rowptr) - 1
        want = np.array([np.diff(g_rowptr)[a_col[a_rowptr[r]:a_rowptr[r + 1]]].sum() for r in range(nrows)], dtype=np.int64)
        ub = torch.full((nrows + 2,), -1, dtype=torch.int64, device="cuda")
        d_rp, d_col, d_g = _dev((a_rowptr + base).astype(Ti)), _dev((a_col + base).astype(Ti)), _dev(g_rowptr)
        hp._capi.call(f"hpcla_spgemm_ub_{which}", d_rp.data_ptr(), d_col.data_ptr(), nrows, base, d_g.data_ptr(), ub.data_ptr(),
                      _stream())
        torch.cuda.synchronize()
        got = ub.cpu().numpy()
        np.testing.assert_array_equal(got[:nrows], want)
        assert got[nrows:].tolist() == [-1, -1], "the kernel wrote past nrows"
    assert want.tolist() == [0, 3 * 2 ** 30, 2 ** 30] and want[1] > np.iinfo(np.int32).max


@pytest.mark.parametrize("family", list(ROW_FAMILIES))
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("which", ["i32", "i64"])
def test_every_admissible_bin_gives_the_reference_bits(hp, caps, which, base, family):
    """Bin b gets ALL rows with ub <= cap[b] -- short rows through the larger kernels too, as the header allows -- in
    descending row order.  (Never a row above the bin's cap: see the module docstring.)  big_columns is the case that
    found the 64-lane register kernel dropping the product in slot 63 of column 2^58 - 1: its sort key is all ones, which
    the kernel used to read as "no product"."""
    c, ref = _family(family, caps)
    d = _DeviceCase(c, which, base)
    nrows = len(c["ub"])
    ub_prefix, total = _slots(c["ub"], range(nrows))
    ran = 0
    for b, cap in enumerate(caps):
        rows = np.flatnonzero(c["ub"] <= cap)[::-1]
        assert np.all(c["ub"][rows] <= cap)
        if len(rows):
            _run_numeric_and_check(hp, d, c, ref, b, rows, ub_prefix, total, f"{family} {which} base {base} bin {b}")
            ran += 1
    assert ran >= 2 and len(rows) == nrows               # the last bin admits every row


@pytest.mark.parametrize("b", range(len(ROWS_PER_WORKGROUP)))
@pytest.mark.parametrize("which", ["i32", "i64"])
def test_partial_workgroups(hp, orc, caps, which, b):
    """n_list = 1, G - 1, G, G + 1 for G rows per workgroup (and 0: nothing is written), rows of the bin's own length, listed
    in a shuffled order, their slots laid out in another shuffled order (offsets not monotone in the row number)."""
    G = ROWS_PER_WORKGROUP[b]
    c = bin_rows(caps, b, G + 1)
    assert c["ub"].max() <= caps[b]
    args = (c["a_rowptr"], c["a_col"], c["a_val"], c["g_rowptr"], c["g_col"], c["g_val"])
    ref = gustavson_ref(*args)
    for got, want in zip(ref, orc.spgemm(*args, c["ncols"])):
        np.testing.assert_array_equal(got, want)
    base = 1 if which == "i64" else 0
    d = _DeviceCase(c, which, base)
    rng = np.random.default_rng(b)
    ub_prefix, total = _slots(c["ub"], rng.permutation(G + 1))
    for n_list in sorted({0, 1, G - 1, G, G + 1}):
        rows = rng.permutation(G + 1)[:n_list]
        _run_numeric_and_check(hp, d, c, ref, b, rows, ub_prefix, total, f"bin {b} {which} n_list {n_list}")


@pytest.mark.parametrize("lens", [(6144,), (65, 0, 64), (1, 6144, 0, 63), (64, 0, 65, 1, 63)], ids=lambda v: f"nrows{len(v)}")
def test_compact(hp, lens):
    """hpcla_spgemm_compact (one wavefront per row, four rows per workgroup) against numpy slicing: rows of 0, 1, 63, 64, 65
    and 6144 entries, upper-bound slots longer than the rows and laid out in a shuffled order."""
    import torch
    rng = np.random.default_rng(len(lens))
    lens = np.array(lens, dtype=np.int64)
    nrows = len(lens)
    ub = lens + rng.integers(0, 5, size=nrows)
    ub_prefix, total = _slots(ub, rng.permutation(nrows))
    col_tmp, val_tmp = rng.integers(0, 2 ** 58, size=total), order_sensitive(rng, total)
    c_rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(c_rowptr[-1])
    c_col = torch.full((nnz + 4,), -1, dtype=torch.int64, device="cuda")
    c_val = torch.full((nnz + 4,), float("nan"), dtype=torch.float64, device="cuda")
    d_rp, d_prefix, d_col, d_val = _dev(c_rowptr), _dev(ub_prefix), _dev(col_tmp), _dev(val_tmp)
    hp._capi.call("hpcla_spgemm_compact", d_rp.data_ptr(), d_prefix.data_ptr(), nrows, d_col.data_ptr(), d_val.data_ptr(),
                  c_col.data_ptr(), c_val.data_ptr(), _stream())
    torch.cuda.synchronize()
    take = np.concatenate([np.arange(ub_prefix[r], ub_prefix[r] + lens[r]) for r in range(nrows)])
    np.testing.assert_array_equal(c_col.cpu().numpy(), np.concatenate([col_tmp[take], np.full(4, -1)]))
    np.testing.assert_array_equal(c_val.cpu().numpy().view(np.uint64),
                                  np.concatenate([val_tmp[take], np.full(4, np.nan)]).view(np.uint64))


@pytest.mark.parametrize("ptr_is_i64", [0, 1])
@pytest.mark.parametrize("name,counts", mapped_lists(), ids=[n for n, _ in mapped_lists()])
def test_mapped_lists_raw(hp, name, counts, ptr_is_i64):
    """hpcla_spgemm_numeric_mapped_f64 on hand-made lists (the host layer cannot produce an int64 list pointer below 2^31
    products, the raw entry takes one at any size): every pass variant as a full and as a last pass, entries that start, end
    and continue on pass boundaries, trailing blocks of one entry."""
    import torch
    m = mapped_case(name, counts)
    want = mapped_ref(m["pair_ptr"], m["pairs"], m["a_val"], m["g_val"])
    nnz_c = len(counts)
    ptr = _dev(m["pair_ptr"].astype(np.int64 if ptr_is_i64 else np.int32))
    c_val = torch.full((nnz_c + 5,), float("nan"), dtype=torch.float64, device="cuda")
    pairs, a_val, g_val = _dev(m["pairs"]), _dev(m["a_val"]), _dev(m["g_val"])
    assert pairs.data_ptr() % 8 == 0
    hp._capi.call("hpcla_spgemm_numeric_mapped_f64", ptr.data_ptr(), ptr_is_i64, pairs.data_ptr(), a_val.data_ptr(),
                  g_val.data_ptr(), c_val.data_ptr(), nnz_c, _stream())
    torch.cuda.synchronize()
    got = c_val.cpu().numpy()
    bad = np.flatnonzero(got[:nnz_c].view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, f"{name}: {len(bad)} entries differ, first {bad[:5].tolist()} with {np.asarray(counts)[bad[:5]].tolist()} products"
    assert np.all(np.isnan(got[nnz_c:])), "the kernel wrote past nnz_c"


def test_spgemm_argument_errors(hp):
    """Every entry refuses bad arguments with a status (no kernel is launched) and accepts empty work with null pointers."""
    import torch
    HPCLAError = hp._capi.HPCLAError
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    s = _stream()

    def numeric(sfx, b, n_list, row_list=p, a_rowptr=p):
        hp._capi.call(f"hpcla_spgemm_numeric_{sfx}", b, a_rowptr, p, p, 0, p, p, p, row_list, n_list, p, p, p, p, s)

    for sfx in ("i32", "i64"):
        for b in (-1, 5):
            with pytest.raises(HPCLAError, match="bad bin"):
                numeric(sfx, b, 1)
        with pytest.raises(HPCLAError, match="negative"):
            numeric(sfx, 0, -1)
        with pytest.raises(HPCLAError, match="null"):
            numeric(sfx, 0, 1, row_list=None)
        with pytest.raises(HPCLAError, match="negative"):
            hp._capi.call(f"hpcla_spgemm_ub_{sfx}", p, p, -1, 0, p, p, s)
        with pytest.raises(HPCLAError, match="null"):
            hp._capi.call(f"hpcla_spgemm_ub_{sfx}", None, p, 1, 0, p, p, s)
        for b in range(5):
            numeric(sfx, b, 0, row_list=None, a_rowptr=None)
        hp._capi.call(f"hpcla_spgemm_ub_{sfx}", None, None, 0, 0, None, None, s)
    with pytest.raises(HPCLAError, match="negative"):
        hp._capi.call("hpcla_spgemm_compact", p, p, -1, p, p, p, p, s)
    with pytest.raises(HPCLAError, match="null"):
        hp._capi.call("hpcla_spgemm_compact", None, p, 1, p, p, p, p, s)
    hp._capi.call("hpcla_spgemm_compact", None, None, 0, None, None, None, None, s)
    for is64 in (0, 1):
        with pytest.raises(HPCLAError, match="negative"):
            hp._capi.call("hpcla_spgemm_numeric_mapped_f64", p, is64, p, p, p, p, -1, s)
        with pytest.raises(HPCLAError, match="null"):
            hp._capi.call("hpcla_spgemm_numeric_mapped_f64", p, is64, None, p, p, p, 1, s)
        assert p % 8 == 0
        with pytest.raises(HPCLAError, match="aligned"):
            hp._capi.call("hpcla_spgemm_numeric_mapped_f64", p, is64, ctypes.c_void_p(p + 4), p, p, p, 1, s)
        hp._capi.call("hpcla_spgemm_numeric_mapped_f64", None, is64, None, None, None, None, 0, s)
    torch.cuda.synchronize()
    assert bool((buf == 0).all())


def _csr_of(M):
    return M.rowptr.astype(np.int64), M.col_indices[M.colval.astype(np.int64)], M.nzval.cpu().numpy()


def _oracle_product(orc, a, b, ncols):
    """orc.spgemm of host CSR a = (rowptr, global cols, vals, ncols) and b, the way the host layer forms it: A's columns
    compressed to the B rows it names, those rows gathered."""
    a_rp, a_col, a_val = a
    b_rp, b_col, b_val = b
    ci = np.unique(a_col)
    g_rowptr = np.concatenate([[0], np.cumsum(np.diff(b_rp)[ci])]).astype(np.int64)
    sel = np.concatenate([np.arange(b_rp[r], b_rp[r + 1]) for r in ci])
    return orc.spgemm(a_rp, np.searchsorted(ci, a_col), a_val, g_rowptr, b_col[sel], b_val[sel], ncols)


def _five_products(hp, orc, backend, a, b, nk, ncols, what):
    """Symbolic, direct-write, list build, lists, lists: values scaled by powers of two (exact in every product and sum)."""
    from hpcla_amd.matmat import get_matrix_plan
    w_rp, w_col, w_val = _oracle_product(orc, a, b, ncols)
    mk = lambda m, n, f: hp.HPCSparseMatrix_local(m[0], m[1], m[2] * f, n, backend)   # noqa: E731
    A = mk(a, nk, 1.0)
    B = mk(b, ncols, 1.0)
    for step, (fa, fb) in enumerate(((1.0, 1.0), (2.0, 1.0), (1.0, 4.0), (2.0, 4.0), (0.5, 0.25))):
        rp, col, val = _csr_of(mk(a, nk, fa) @ mk(b, ncols, fb))
        np.testing.assert_array_equal(rp, w_rp, err_msg=f"{what}: product {step}")
        np.testing.assert_array_equal(col, w_col, err_msg=f"{what}: product {step}")
        np.testing.assert_array_equal(val.view(np.uint64), (fa * fb * w_val).view(np.uint64), err_msg=f"{what}: product {step}")
    res = get_matrix_plan(A, B).cache["symbolic"]["result"]
    assert res["map"] is not None, "the product lists were not built"
    assert res["repeats"] == 4
    return A, B, (w_rp, w_col, w_val)


@pytest.mark.parametrize("which", ["i32", "i64"])
def test_host_layer_at_the_row_limit(hp, orc, caps, gpu_backend_i32, gpu_backend_i64, which, monkeypatch):
    """A @ B with a row of exactly caps[-1] candidates in 6144 distinct columns, one of caps[-1] candidates in ONE column and
    ordinary rows; the same with one candidate more is refused by name and leaves nothing half-built behind."""
    from hpcla_amd.matmat import _plan_cache, clear_matrix_plan_cache, get_matrix_plan
    backend = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    cap = caps[-1]
    clear_matrix_plan_cache()
    rng = np.random.default_rng(cap)
    # B: rows 0 .. cap-1 hold one entry each in column 7; rows cap .. cap+47 hold cap / 48 entries each, disjoint;
    # row cap+48 holds one entry more (used by the refused product only); then 20 ordinary rows
    per = cap // 48
    assert per * 48 == cap
    nb, ncols = cap + 48 + 1 + 20, cap + 40
    b_rows = [np.array([7])] * cap + [np.arange(per * i, per * (i + 1)) + 20 for i in range(48)] + [np.array([3])]
    b_rows += [np.sort(rng.permutation(ncols)[:rng.integers(1, 9)]) for _ in range(20)]
    b_rp = np.concatenate([[0], np.cumsum([len(r) for r in b_rows])]).astype(np.int64)
    b = (b_rp, np.concatenate(b_rows).astype(np.int64), order_sensitive(rng, int(b_rp[-1])))

    def make_a(extra):
        rows = [np.sort(rng.permutation(20)[:5]) + cap + 49 for _ in range(6)]
        rows.insert(2, np.arange(cap))                                     # one_column: ub = nk = cap
        rows.insert(4, np.arange(cap, cap + 48 + (1 if extra else 0)))     # distinct: ub = cap (+ 1)
        rows.insert(5, np.zeros(0, dtype=np.int64))
        rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        return rp, np.concatenate(rows).astype(np.int64), order_sensitive(rng, int(rp[-1]))

    a = make_a(False)
    ub = np.array([np.diff(b_rp)[a[1][a[0][r]:a[0][r + 1]]].sum() for r in range(len(a[0]) - 1)])
    assert ub[2] == cap == ub[4] and ub.max() == cap and ub[5] == 0
    A, B, (w_rp, w_col, w_val) = _five_products(hp, orc, backend, a, b, nb, ncols, f"row limit {which}")
    assert np.diff(w_rp)[2] == 1 and np.diff(w_rp)[4] == cap
    monkeypatch.setenv("HPCLA_SPGEMM_MAP", "0")                            # and without the lists: the numeric kernels
    clear_matrix_plan_cache()
    for _ in range(3):
        np.testing.assert_array_equal(_csr_of(A @ B)[2].view(np.uint64), w_val.view(np.uint64))
    monkeypatch.delenv("HPCLA_SPGEMM_MAP")
    # one candidate more
    a_over = make_a(True)
    A_over = hp.HPCSparseMatrix_local(a_over[0], a_over[1], a_over[2], nb, backend)
    with pytest.raises(NotImplementedError, match=str(cap + 1)):
        A_over @ B
    assert len(_plan_cache) == 2 and "symbolic" not in get_matrix_plan(A_over, B).cache
    assert sum("symbolic" in plan.cache for plan in _plan_cache.values()) == 1      # the valid product's, not the refused one's
    with pytest.raises(NotImplementedError, match=str(cap + 1)):                    # and again: nothing half-built is reused
        A_over @ B
    np.testing.assert_array_equal(_csr_of(A @ B)[2].view(np.uint64), w_val.view(np.uint64))
    clear_matrix_plan_cache()


def test_host_layer_dense_accumulation_runs_multi_chunk_lists(hp, orc, caps, gpu_backend_i32):
    """100 full rows of 300 entries times 300 rows over the same 20 columns: ub = 6000 per row (the workgroup hash kernel),
    2000 result entries of 300 products each -- every 256-entry block of the lists streams 75 passes of 1024 products."""
    from hpcla_amd.matmat import clear_matrix_plan_cache
    clear_matrix_plan_cache()
    rng = np.random.default_rng(300)
    m, k, n = 100, 300, 50
    assert caps[-2] < 20 * k <= caps[-1] and (256 * k) // 1024 == 75
    a = (np.arange(0, m * k + 1, k, dtype=np.int64), np.tile(np.arange(k, dtype=np.int64), m), order_sensitive(rng, m * k))
    cols = np.sort(rng.permutation(n)[:20]).astype(np.int64)
    b = (np.arange(0, 20 * k + 1, 20, dtype=np.int64), np.tile(cols, k), order_sensitive(rng, 20 * k))
    _, _, (w_rp, _, _) = _five_products(hp, orc, gpu_backend_i32, a, b, k, n, "dense accumulation")
    assert w_rp[-1] == 2000
    clear_matrix_plan_cache()
