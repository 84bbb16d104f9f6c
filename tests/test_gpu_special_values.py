"""Inf, NaN, signed zeros, denormals and finfo.max through every kernel family (inputs: tests/_special_values_cases.py,
validated on the CPU in tests/test_special_values_cases.py).

Why: every fast path here pads, clamps or re-reads (lanes past a row's end hold a zero value and column 0, odd-k SpMM reads
the padding double of a B row, gram pads rows with zeros ...).  On finite data ``0 * x`` adds nothing; with ``x = Inf`` it is a
NaN, and ``acc = first product`` instead of ``acc = 0; acc += product`` shows as a ``-0.0`` where the reference gives ``+0.0``.
And NaN is part of the transport protocol: an expired halo wait poisons its rows, and the caller learns of it through the
reductions -- a kernel that drops a NaN turns a failed exchange into a plausible number.

RULE E (exact): families whose contract is the reference's bits.  ``assert_array_equal`` against the oracle (NaN equals
NaN, payloads open) AND the sign of every expected zero.  Outputs are pre-filled with the finite sentinel 7.0, so an
unwritten element cannot pass as an expected NaN.

RULE C (class + bound): families that sum in another order by design (long rows, gram, dense A*x / A'x, reductions).  Their
operands hold no finfo.max and only moderate finite magnitudes, so the class of each output follows from the list of
products in any order (any NaN product, or +Inf and -Inf -> NaN; only +Inf -> +Inf; only -Inf -> -Inf); finite outputs meet
the bound the family's existing test uses (1e-12 * sum |a||b|; 1 ulp of float32(exact) for the Float32 gram).  The sign of an
exact zero is NOT asserted under rule C: a kernel that starts from its first product (gemv_skinny) legitimately keeps a -0.0.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _special_values_cases as sv  # noqa: E402

pytestmark = pytest.mark.gpu
SENT = 7.0
PASS = 464                   # entries of one wave pass of the row-gather kernels (csrc/rowgather_t.h)


def _torch():
    import torch
    return torch


def _t(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).to("cuda")


def _s():
    return _torch().cuda.current_stream().cuda_stream


def _full(shape, T):
    torch = _torch()
    return torch.full(shape, SENT, dtype=torch.float64 if np.dtype(T) == np.float64 else torch.float32, device="cuda")


def _sfx(Ti):
    return "i32" if Ti == np.int32 else "i64"


def _dt(T):
    return "f64" if np.dtype(T) == np.float64 else "f32"


def same(got, want, what=""):
    """Rule E."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and not np.array_equal(got, want, equal_nan=True):
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(len(want), -1).all(axis=1))
        print(f"{what}: differing rows {bad[:20]} of {len(bad)}")
    np.testing.assert_array_equal(got, want, err_msg=what)
    z = want == 0
    assert np.array_equal(np.signbit(got[z]), np.signbit(want[z])), \
        f"{what}: sign of zero differs at {np.flatnonzero((np.signbit(got) != np.signbit(want)) & z)[:20]}"


def classed(got, cls, ref, bound, what="", rtol=1e-12):
    """Rule C."""
    got = np.asarray(got, dtype=np.float64)
    gc = sv.class_of_values(got)
    assert np.array_equal(gc, cls), f"{what}: class differs at {np.argwhere(gc != cls)[:20].tolist()}"
    fin = cls == sv.FINITE
    err = np.abs(got[fin] - np.asarray(ref)[fin])
    assert np.all(err <= rtol * np.asarray(bound)[fin]), f"{what}: {err.max()}"


def scalar_classed(got, products, what=""):
    p = np.asarray(products, dtype=np.float64).ravel()
    cls = sv.classes_of(p)
    fin = np.where(np.isfinite(p), p, 0.0)
    classed(np.array([got]), np.array([cls]), np.array([math.fsum(fin)]), np.array([np.abs(fin).sum()]), what)


def _oracle_mm(orc, rowptr, col, vals, B):
    with np.errstate(all="ignore"):
        return orc.spmm(rowptr.astype(np.int32), col.astype(np.int32), vals, B)


def _oracle_mv(orc, rowptr, col, vals, x):
    with np.errstate(all="ignore"):
        return orc.spmv(rowptr.astype(np.int32), col.astype(np.int32), vals, np.ascontiguousarray(x))


def _long_rows_keep_their_classes(want):
    """The expected values of the rows of 465 ... 3 000 entries are finite, +Inf, -Inf, NaN and an exact zero (LONG_CLASS), not
    NaN throughout: the multi-pass code they reach is held to more than NaN propagation."""
    want = np.asarray(want).reshape(sv.NROWS, -1)
    for r, cls in sv.LONG_CLASS.items():
        assert np.all(sv.class_of_values(want[r]) == cls), (r, want[r])
    assert np.all(want[[5, 63]] != 0) and np.all(want[901] == 0)


@pytest.fixture(scope="module")
def gen():
    """The general structure with its values and 4-column operands for both element types and both rules."""
    rowptr, col = sv.general()
    out = {"rowptr": rowptr, "col": col, "n": sv.NROWS, "nc": sv.NCOLS, "lens": np.diff(rowptr)}
    for T in (np.float64, np.float32):
        out[_dt(T)] = {"vals": sv.values(rowptr, col, T), "B": sv.operand(sv.NCOLS, 4, T), "Bc": sv.operand(sv.NCOLS, 4, T, rule="C")}
    return out


@pytest.fixture(scope="module")
def band():
    rowptr, col, base = sv.banded()
    n = sv.NX * sv.NY
    return {"rowptr": rowptr, "col": col, "n": n, "base": base, "vals": sv.values(rowptr, col, np.float64, base=base),
            "B": sv.operand(n, 4, np.float64), "B16": sv.operand(n, 16, np.float64)}


# ---------------------------------------------------------------------------------------------------------------------
# SpMV, row gather
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_csr_rowgather(hp, orc, gen, Ti, base):
    """hpcla_spmv_csr_f64_{i32,i64}, aligned arrays: the row-gather kernel.  Reached: rows of 465 ... 3000 entries exceed one
    wave pass (asserted against PASS) and their expected sums are finite, +Inf, -Inf, NaN and an exact zero (asserted), short
    rows pad their lanes (value 0, column 0 -- and x[0] is Inf / NaN here).  Rule E, every operand column as x."""
    assert gen["lens"].max() > 6 * PASS and (gen["lens"] == PASS + 1).any() and hp._capi.load().hpcla_spmv_rows_per_block() == 256
    d = gen["f64"]
    rp, cv, nz = _t((gen["rowptr"] + base).astype(Ti)), _t((gen["col"] + base).astype(Ti)), _t(d["vals"])
    assert cv.data_ptr() % 16 == 0 and nz.data_ptr() % 32 == 0
    want = _oracle_mm(orc, gen["rowptr"], gen["col"], d["vals"], d["B"])
    _long_rows_keep_their_classes(want)
    for c in range(4):
        x, y = _t(d["B"][:, c]), _full((gen["n"],), np.float64)
        hp._capi.call(f"hpcla_spmv_csr_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), x.data_ptr(), y.data_ptr(),
                      gen["n"], len(d["vals"]), base, _s())
        same(y.cpu().numpy(), want[:, c], f"column {c}")


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_unaligned_fallback(hp, orc, gen, Ti):
    """colval / nzval one element into a larger buffer (nzval not 32-byte aligned, asserted): the element-per-lane fallback
    kernel of the same entry point.  Rule E."""
    d = gen["f64"]
    rp = _t(gen["rowptr"].astype(Ti))
    cv = _t(np.concatenate([[0], gen["col"]]).astype(Ti))[1:]
    nz = _t(np.concatenate([[np.nan], d["vals"]]))[1:]
    assert nz.data_ptr() % 32 != 0 and cv.data_ptr() % 16 != 0
    want = _oracle_mm(orc, gen["rowptr"], gen["col"], d["vals"], d["B"])
    for c in range(4):
        x, y = _t(d["B"][:, c]), _full((gen["n"],), np.float64)
        hp._capi.call(f"hpcla_spmv_csr_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), x.data_ptr(), y.data_ptr(),
                      gen["n"], len(d["vals"]), 0, _s())
        same(y.cpu().numpy(), want[:, c], f"column {c}")


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_split_specials_straddle_n_own(hp, orc, gen, Ti):
    """hpcla_spmv_split_f64_*: x_own | x_ghost with +Inf in the last own entry and NaN in the first ghost entry (both columns
    are referenced: asserted), without a block list and with two complementary block lists (rows of unlisted blocks keep the
    sentinel).  Rule E."""
    d = gen["f64"]
    n = gen["n"]
    used = np.bincount(gen["col"], minlength=gen["nc"]) > 0
    n_own = next(c for c in range(sv.BAND[1] + 100, gen["nc"]) if used[c - 1] and used[c])       # behind the long rows' band
    x = d["B"][:, 0].copy()
    x[n_own - 1], x[n_own] = np.inf, np.nan
    want = _oracle_mv(orc, gen["rowptr"], gen["col"], d["vals"], x)
    _long_rows_keep_their_classes(want)
    rp, cv, nz = _t(gen["rowptr"].astype(Ti)), _t(gen["col"].astype(Ti)), _t(d["vals"])
    xo, xg = _t(x[:n_own]), _t(x[n_own:])
    fn = f"hpcla_spmv_split_f64_{_sfx(Ti)}"
    y = _full((n,), np.float64)
    hp._capi.call(fn, rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xo.data_ptr(), xg.data_ptr(), n_own, y.data_ptr(), n,
                  len(d["vals"]), 0, None, 0, _s())
    same(y.cpu().numpy(), want, "no list")
    rpb = hp._capi.load().hpcla_spmv_rows_per_block()
    nblk = (n + rpb - 1) // rpb
    even, odd = np.arange(0, nblk, 2, dtype=np.int32), np.arange(1, nblk, 2, dtype=np.int32)
    y.fill_(SENT)
    lst = _t(even)
    hp._capi.call(fn, rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xo.data_ptr(), xg.data_ptr(), n_own, y.data_ptr(), n,
                  len(d["vals"]), 0, lst.data_ptr(), len(even), _s())
    got = y.cpu().numpy()
    for b in range(nblk):
        sl = slice(b * rpb, min(n, (b + 1) * rpb))
        if b % 2 == 0:
            same(got[sl], want[sl], f"block {b}")
        else:
            assert np.all(got[sl] == SENT)
    lst2 = _t(odd)
    hp._capi.call(fn, rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xo.data_ptr(), xg.data_ptr(), n_own, y.data_ptr(), n,
                  len(d["vals"]), 0, lst2.data_ptr(), len(odd), _s())
    same(y.cpu().numpy(), want, "both lists")


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_dist_dot_epilogue(hp, orc, gen, Ti):
    """hpcla_spmv_dist_dot_f64_* with plan = comm = NULL on the general rows padded with empty rows to a square matrix (the
    epilogue pairs x[r] with y[r]): y under rule E; the x.y scalar under rule C on the rule-C operand (its class follows from
    the products x[r] * y[r]: NaN for all four columns, the NaN rows of y see to that), then with plain values a finite scalar
    and an infinite one."""
    d = gen["f64"]
    nc = gen["nc"]
    rowptr = np.concatenate([gen["rowptr"], np.full(nc - gen["n"], gen["rowptr"][-1])])
    rp, cv, nz = _t(rowptr.astype(Ti)), _t(gen["col"].astype(Ti)), _t(d["vals"])
    lib = hp._capi.load()
    torch = _torch()
    work = torch.empty(lib.hpcla_spmv_dot_work_bytes(nc) // 8 + 1, dtype=torch.float64, device="cuda")
    for c in range(4):
        x = d["Bc"][:, c]
        want = _oracle_mv(orc, rowptr, gen["col"], d["vals"], x)
        xd, y = _t(x), _full((nc,), np.float64)
        out = _full((1,), np.float64)
        hp._capi.call(f"hpcla_spmv_dist_dot_f64_{_sfx(Ti)}", None, None, rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xd.data_ptr(), nc,
                      y.data_ptr(), nc, len(d["vals"]), 0, None, 0, None, 0, out.data_ptr(), work.data_ptr(), _s())
        same(y.cpu().numpy(), want, f"column {c}")
        with np.errstate(all="ignore"):
            scalar_classed(out.item(), x * want, f"x.y column {c}")
    # a FINITE scalar and an Inf one through the same entry: plain values, the -0.0 column as x; then +Inf in an x entry that no
    # matrix column reads (y unchanged) and whose y is not zero
    plain = sv.values(gen["rowptr"], gen["col"], np.float64, special=False)
    nz = _t(plain)
    x = d["Bc"][:, 3].copy()
    used = np.bincount(gen["col"], minlength=nc) > 0
    want = _oracle_mv(orc, rowptr, gen["col"], plain, x)
    r_inf = next(r for r in range(gen["n"]) if not used[r] and want[r] != 0)
    for tag, cls in (("finite", sv.FINITE), ("inf", None)):
        if tag == "inf":
            x[r_inf] = np.inf
            want = _oracle_mv(orc, rowptr, gen["col"], plain, x)
        assert np.all(np.isfinite(want))
        xd, y, out = _t(x), _full((nc,), np.float64), _full((1,), np.float64)
        hp._capi.call(f"hpcla_spmv_dist_dot_f64_{_sfx(Ti)}", None, None, rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xd.data_ptr(), nc,
                      y.data_ptr(), nc, len(plain), 0, None, 0, None, 0, out.data_ptr(), work.data_ptr(), _s())
        same(y.cpu().numpy(), want, f"plain values, {tag}")
        with np.errstate(all="ignore"):
            scalar_classed(out.item(), x * want, f"x.y plain values, {tag}")
        assert math.isfinite(out.item()) if tag == "finite" else math.isinf(out.item())


# ---------------------------------------------------------------------------------------------------------------------
# 16-bit columns and the packed copy (banded structure)
# ---------------------------------------------------------------------------------------------------------------------
def test_cols16_raw_entries(hp, orc, band):
    """hpcla_cols16_encode_i32 + hpcla_spmv_cols16_f64_i32 and hpcla_spmv_dist_dot_cols16_f64_i32 on the 5-point matrix with
    special values: the encoder reports the copy eligible (asserted: the narrow kernel really ran).  y: rule E; the scalar:
    rule C -- the -0.0 column of the operand with the matrix' clean values is a FINITE sum, the others are not."""
    torch = _torch()
    lib = hp._capi.load()
    n, nnz = band["n"], len(band["col"])
    rp, cv = _t(band["rowptr"].astype(np.int32)), _t(band["col"].astype(np.int32))
    c16 = torch.zeros(lib.hpcla_cols16_padded_len(nnz), dtype=torch.int16, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    hp._capi.call("hpcla_cols16_encode_i32", rp.data_ptr(), cv.data_ptr(), n, nnz, n, 0, None, 0, c16.data_ptr(), bad.data_ptr(), _s())
    assert bad.item() == 0, "the banded structure must be eligible"
    work = torch.empty(lib.hpcla_spmv_dot_work_bytes(n) // 8 + 1, dtype=torch.float64, device="cuda")
    for vals, tag in ((band["vals"], "special values"), (band["base"], "clean values")):
        nz = _t(vals)
        assert nz.data_ptr() % 32 == 0 and c16.data_ptr() % 16 == 0
        want = _oracle_mm(orc, band["rowptr"], band["col"], vals, band["B"])
        for c in range(4):
            x = band["B"][:, c]
            xd, y = _t(x), _full((n,), np.float64)
            hp._capi.call("hpcla_spmv_cols16_f64_i32", rp.data_ptr(), c16.data_ptr(), nz.data_ptr(), xd.data_ptr(), y.data_ptr(), n, nnz, 0,
                          None, 0, _s())
            same(y.cpu().numpy(), want[:, c], f"{tag}, cols16 column {c}")
            if c == 0:
                continue                                     # finfo.max in column 0: the scalar's class would depend on order
            y.fill_(SENT)
            out = _full((1,), np.float64)
            hp._capi.call("hpcla_spmv_dist_dot_cols16_f64_i32", None, None, rp.data_ptr(), cv.data_ptr(), c16.data_ptr(), nz.data_ptr(),
                          xd.data_ptr(), n, y.data_ptr(), n, nnz, 0, None, 0, None, 0, out.data_ptr(), work.data_ptr(), _s())
            same(y.cpu().numpy(), want[:, c], f"{tag}, dist_dot_cols16 column {c}")
            with np.errstate(all="ignore"):
                scalar_classed(out.item(), x * want[:, c], f"{tag}, x.y column {c}")
            if tag == "clean values" and c == 3:
                assert math.isfinite(out.item())


def test_cols16_host_layer_both_paths(hp, orc, band, gpu_backend_i32, monkeypatch):
    """Host layer with HPCLA_NARROW_COLS at its default (plan.cols16 is not None: asserted) and = 0 (None): the same bits as
    each other and as the oracle, A @ x and mul_dot_.  Rule E."""
    torch = _torch()
    n = band["n"]
    x = band["B"][:, 1]
    want = _oracle_mv(orc, band["rowptr"], band["col"], band["vals"], x)
    outs = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("HPCLA_NARROW_COLS", "0")
        else:
            monkeypatch.delenv("HPCLA_NARROW_COLS", raising=False)
        A = hp.HPCSparseMatrix_local(band["rowptr"], band["col"], band["vals"], n, gpu_backend_i32)
        xv = hp.HPCVector.from_global(x, gpu_backend_i32)
        plan = hp.get_vector_plan(A, xv)
        assert (plan.cols16 is not None) == (not off)
        same((A @ xv).local_values(), want, f"A @ x, narrow off = {off}")
        y = xv.similar()
        y.v.fill_(SENT)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        hp.mul_dot_(y, A, xv, out)
        same(y.local_values(), want, f"mul_dot_, narrow off = {off}")
        outs.append(out.cpu().numpy().copy())
    monkeypatch.delenv("HPCLA_NARROW_COLS", raising=False)
    assert np.array_equal(outs[0], outs[1], equal_nan=True)
    hp.clear_plan_cache()


def test_packed_copy_and_its_refusals(hp, orc, band, gpu_backend_i32):
    """A.enable_packed on the 5-point structure with values {4, -1, -0.0, +Inf, a denormal} (one kind of zero, no NaN) and the
    specials in x: enable_packed is True (asserted: the packed kernel ran), A @ x and mul_dot_ under rule E.  The two refusals
    no other test reaches: values holding NaN, and values holding both zeros -> False with the reason, CSR product intact."""
    torch = _torch()
    b = gpu_backend_i32
    n = band["n"]
    rng = np.random.default_rng(8)
    vals = band["base"].copy()
    for v in (-0.0, np.inf, np.finfo(np.float64).tiny / 8):
        vals[rng.choice(len(vals), 300, replace=False)] = v
    assert len(np.unique(vals.view(np.int64))) == 5
    for c in range(4):
        x = band["B"][:, c]
        want = _oracle_mv(orc, band["rowptr"], band["col"], vals, x)
        A = hp.HPCSparseMatrix_local(band["rowptr"], band["col"], vals, n, b)
        xv = hp.HPCVector.from_global(x, b)
        assert A.enable_packed(xv) is True, A.packed_reason
        same((A @ xv).local_values(), want, f"packed A @ x column {c}")
        y = xv.similar()
        y.v.fill_(SENT)
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        hp.mul_dot_(y, A, xv, out)
        same(y.local_values(), want, f"packed mul_dot_ column {c}")
        A.disable_packed()
        same((A @ xv).local_values(), want, f"CSR column {c}")
    x = band["B"][:, 1]
    xv = hp.HPCVector.from_global(x, b)
    for poison, reason in ((np.nan, "NaN"), (0.0, "both -0.0 and +0.0")):
        v2 = vals.copy()
        v2[12345] = poison
        A = hp.HPCSparseMatrix_local(band["rowptr"], band["col"], v2, n, b)
        assert A.enable_packed(xv) is False and reason in A.packed_reason, A.packed_reason
        same((A @ xv).local_values(), _oracle_mv(orc, band["rowptr"], band["col"], v2, x), f"refused ({reason})")
    hp.clear_plan_cache()


# ---------------------------------------------------------------------------------------------------------------------
# long rows (tree order on rows of >= 928 entries)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmv_long_rows(hp, orc, gen, Ti):
    """hpcla_spmv_longrows_f64_* with long_min = 928 and A.enable_long_rows(928): the rows of 1 000 ... 3 000 entries are summed in
    tree order (their number is asserted) -- rule C on the rule-C operand, and their classes are finite non-zero, exact zero,
    +Inf, -Inf and NaN (asserted), so a tree kernel that wrote nothing would leave the main kernel's NaN in a finite row and
    fail; every other row, the 465-entry one included, rule E."""
    torch = _torch()
    d = gen["f64"]
    n, nc = gen["n"], gen["nc"]
    is_long = gen["lens"] >= 928
    n_long = int(is_long.sum())
    assert n_long == 5 and gen["lens"][~is_long].max() == 465
    rp, cv, nz = _t((gen["rowptr"] + 1).astype(Ti)), _t((gen["col"] + 1).astype(Ti)), _t(d["vals"])
    rows = _t(np.flatnonzero(is_long).astype(np.int64))
    work = torch.empty(hp._capi.load().hpcla_spmv_longrows_work_bytes(n_long) // 8, dtype=torch.float64, device="cuda")
    backend = hp.backend_rocm_serial(np.float64, Ti)
    A = hp.HPCSparseMatrix_local(gen["rowptr"], gen["col"], d["vals"], nc, backend)
    assert A.enable_long_rows(928) == n_long
    n_own = 2500
    for c in range(4):
        x = d["Bc"][:, c]
        want = _oracle_mv(orc, gen["rowptr"], gen["col"], d["vals"], x)
        cls, ref, bound = sv.csr_classes(gen["rowptr"], gen["col"], d["vals"], x)
        # the tree sums are really checked: a finite non-zero long row (the main kernel leaves NaN there for the tree kernels to
        # overwrite), an exact zero, +Inf, -Inf and NaN in every column
        assert sorted(cls[is_long].tolist()) == sorted([sv.FINITE, sv.FINITE, sv.PINF, sv.NINF, sv.NAN]) and ref[63] != 0
        xo, xg = _t(x[:n_own]), _t(x[n_own:])
        y = _full((n,), np.float64)
        hp._capi.call(f"hpcla_spmv_longrows_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xo.data_ptr(), xg.data_ptr(),
                      n_own, y.data_ptr(), n, len(d["vals"]), 1, rows.data_ptr(), n_long, 928, work.data_ptr(), _s())
        for got, tag in ((y.cpu().numpy(), "raw"), ((A @ hp.HPCVector.from_global(x, backend)).local_values(), "host")):
            same(got[~is_long], want[~is_long], f"{tag} column {c}, short rows")
            classed(got[is_long], cls[is_long], ref[is_long], bound[is_long], f"{tag} column {c}, long rows")
    hp.clear_plan_cache()


# ---------------------------------------------------------------------------------------------------------------------
# SpMM, row-major B
# ---------------------------------------------------------------------------------------------------------------------
def _padded(M, pitch, fill=np.nan):
    out = np.full((M.shape[0], pitch), fill, dtype=M.dtype)
    out[:, :M.shape[1]] = M
    return out


@pytest.mark.parametrize("k", [3, 4, 7, 8, 16, 17, 40])
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmm_rowmajor_tight_pitch(hp, orc, gen, k, Ti):
    """hpcla_spmm_csr_f64_* and hpcla_spmm_split_f64_* on the pitch k: even k (4, 8, 16, 40) takes the 16-byte vector kernel (16:
    C leaves through LDS), odd k on its own odd pitch (3, 7, 17) the generic one-column-per-lane kernel in its group sizes;
    rows of 2 049 and 3 000 entries exceed CHUNK_MM = 1984 (asserted) and their expected sums are +Inf and -Inf, next to finite,
    NaN and exact-zero long rows (asserted).  Row- and column-major C (hpcla_spmm_split_ccol_f64_*).  Rule E."""
    assert gen["lens"].max() > 1984
    vals = gen["f64"]["vals"]
    n, nc, nnz = gen["n"], gen["nc"], len(vals)
    B = sv.operand(nc, k, np.float64)
    want = _oracle_mm(orc, gen["rowptr"], gen["col"], vals, B)
    _long_rows_keep_their_classes(want)
    rp, cv, nz, Bd = _t(gen["rowptr"].astype(Ti)), _t(gen["col"].astype(Ti)), _t(vals), _t(B)
    ROW, COL = hp._capi.LAYOUT_ROW, hp._capi.LAYOUT_COL
    C = _full((n, k), np.float64)
    hp._capi.call(f"hpcla_spmm_csr_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bd.data_ptr(), k, ROW, C.data_ptr(), k,
                  ROW, n, nnz, k, 0, _s())
    same(C.cpu().numpy(), want, "csr, row-major C")
    n_own = 2500
    Bo, Bg = _t(B[:n_own]), _t(B[n_own:])
    C.fill_(SENT)
    hp._capi.call(f"hpcla_spmm_split_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bo.data_ptr(), k, Bg.data_ptr(), k, n_own,
                  C.data_ptr(), k, n, nnz, k, 0, None, 0, _s())
    same(C.cpu().numpy(), want, "split, row-major C")
    ldc = n + 2
    Cc = _full((k, ldc), np.float64)
    hp._capi.call(f"hpcla_spmm_split_ccol_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bo.data_ptr(), k, Bg.data_ptr(), k,
                  n_own, Cc.data_ptr(), ldc, n, nnz, k, 0, None, 0, _s())
    got = Cc.cpu().numpy()
    same(got[:, :n].T, want, "split, column-major C")
    assert np.all(got[:, n:] == SENT)


@pytest.mark.parametrize("k", [3, 15])
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmm_rowmajor_odd_k_on_padded_pitch(hp, orc, gen, k, Ti):
    """Odd k on the even pitches k + 1 and k + 3: the vector kernel reads the padding double of every B row it gathers (NaN
    here, as in test_spmm_bit_exact_padded_pitch) and never stores it into a real column.  C's padding keeps the sentinel, or
    is the documented 0.0 in column k where ldc == k + 1 <= 16.  Row-major and column-major C, unsplit and split entry.  Rule E."""
    vals = gen["f64"]["vals"]
    n, nc, nnz = gen["n"], gen["nc"], len(vals)
    B = sv.operand(nc, k, np.float64)
    want = _oracle_mm(orc, gen["rowptr"], gen["col"], vals, B)
    _long_rows_keep_their_classes(want)
    rp, cv, nz = _t(gen["rowptr"].astype(Ti)), _t(gen["col"].astype(Ti)), _t(vals)
    ROW, COL = hp._capi.LAYOUT_ROW, hp._capi.LAYOUT_COL
    for ld in (k + 1, k + 3):
        Bd = _t(_padded(B, ld))
        C = _full((n, ld), np.float64)
        hp._capi.call(f"hpcla_spmm_csr_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bd.data_ptr(), ld, ROW, C.data_ptr(),
                      ld, ROW, n, nnz, k, 0, _s())
        got = C.cpu().numpy()
        same(got[:, :k], want, f"pitch {ld}, row-major C")
        assert np.all((got[:, k:] == SENT) | (got[:, k:] == 0.0)) and np.all(got[:, k + 1:] == SENT), "padding of C"
        if ld != k + 1:
            assert np.all(got[:, k:] == SENT)
        ldc = n + 3
        Cc = _full((k, ldc), np.float64)
        hp._capi.call(f"hpcla_spmm_csr_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bd.data_ptr(), ld, ROW, Cc.data_ptr(),
                      ldc, COL, n, nnz, k, 0, _s())
        got = Cc.cpu().numpy()
        same(got[:, :n].T, want, f"pitch {ld}, column-major C")
        assert np.all(got[:, n:] == SENT)
    # split entry: own rows on the pitch k + 1, ghost rows on the pitch k + 3 (their padding doubles are NaN too)
    n_own = 2500
    Bo, Bg = _t(_padded(B[:n_own], k + 1)), _t(_padded(B[n_own:], k + 3))
    C = _full((n, k + 3), np.float64)
    hp._capi.call(f"hpcla_spmm_split_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bo.data_ptr(), k + 1, Bg.data_ptr(), k + 3,
                  n_own, C.data_ptr(), k + 3, n, nnz, k, 0, None, 0, _s())
    got = C.cpu().numpy()
    same(got[:, :k], want, "split, padded pitches")
    assert np.all(got[:, k:] == SENT)


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmm_panel_accumulate_continues_from_special_values(hp, gen, Ti):
    """hpcla_spmm_panel_* with accumulate = 1 on a C that already holds Inf, NaN and -0.0: every C(r, c) CONTINUES from its
    value entry by entry -- a numpy loop with separately rounded multiply and add.  Here -0.0 is a legitimate result (a row
    of -0.0 products added to -0.0).  Rule E."""
    vals = gen["f64"]["vals"]
    B = gen["f64"]["B"]
    n, nc, k = gen["n"], gen["nc"], 4
    rng = np.random.default_rng(9)
    C0 = rng.random((n, k)) - 0.5
    for v in (np.inf, -np.inf, np.nan, -0.0, 0.0):
        C0[rng.choice(n, 60, replace=False), rng.integers(0, k, 60)] = v
    for r in sv.LONG:                                         # the long rows continue from ordinary numbers, 901 from -0.0
        C0[r] = rng.random(k) + 0.25
    C0[[10, 11, 701, 901]] = -0.0
    want = C0.copy()
    rowptr, col = gen["rowptr"], gen["col"]
    with np.errstate(all="ignore"):
        for r in range(n):
            acc = want[r].copy()
            for j in range(rowptr[r], rowptr[r + 1]):
                acc = acc + vals[j] * B[col[j]]
            want[r] = acc
    assert np.all(np.signbit(want[901]) & (want[901] == 0))
    for r, cls in sv.LONG_CLASS.items():
        assert np.all(sv.class_of_values(want[r]) == cls)
    rp, cv, nz, Bd, C = _t(rowptr.astype(Ti)), _t(col.astype(Ti)), _t(vals), _t(B), _t(C0)
    hp._capi.call(f"hpcla_spmm_panel_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bd.data_ptr(), k, None, k, nc,
                  C.data_ptr(), k, n, len(vals), k, 0, 1, _s())
    same(C.cpu().numpy(), want, "panel accumulate")


# ---------------------------------------------------------------------------------------------------------------------
# run tiles (banded structure, k = 16)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_spmm_run_tiles(hp, orc, band, Ti):
    """hpcla_spmm_runs_build_* + hpcla_spmm_runs_k16_f64_* and hpcla_spmm_runs_colmajor_k16_f64_* on the 5-point matrix: every
    block fits (n_fit == number of blocks > 0, asserted), so B rows are staged in LDS and multiplied from there.  Rule E."""
    torch = _torch()
    lib = hp._capi.load()
    n, k, nnz = band["n"], 16, len(band["col"])
    B = band["B16"]
    want = _oracle_mm(orc, band["rowptr"], band["col"], band["vals"], B)
    rp, cv, nz = _t(band["rowptr"].astype(Ti)), _t(band["col"].astype(Ti)), _t(band["vals"])
    desc = torch.empty(lib.hpcla_spmm_runs_desc_bytes(n), dtype=torch.uint8, device="cuda")
    n_fit = ctypes.c_int64(-1)
    hp._capi.call(f"hpcla_spmm_runs_build_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), n, nnz, 0, n, desc.data_ptr(), ctypes.byref(n_fit), _s())
    rpb = lib.hpcla_spmm_rows_per_block()
    assert n_fit.value == (n + rpb - 1) // rpb > 0
    Bd = _t(B)
    C = _full((n, k), np.float64)
    hp._capi.call(f"hpcla_spmm_runs_k16_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bd.data_ptr(), None, n, C.data_ptr(), n,
                  nnz, 0, desc.data_ptr(), None, 0, _s())
    same(C.cpu().numpy(), want, "run tiles, row-major")
    ldb, ldc = n + 2, n + 4
    Bc = _t(_padded(np.ascontiguousarray(B.T), ldb))
    Cc = _full((k, ldc), np.float64)
    assert Bc.data_ptr() % 16 == 0
    hp._capi.call(f"hpcla_spmm_runs_colmajor_k16_f64_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bc.data_ptr(), ldb, None, 16, n,
                  Cc.data_ptr(), ldc, n, nnz, 0, desc.data_ptr(), None, 0, _s())
    got = Cc.cpu().numpy()
    same(got[:, :n].T, want, "run tiles, column-major")
    assert np.all(got[:, n:] == SENT)


# ---------------------------------------------------------------------------------------------------------------------
# lanes = rows (column-major blocks) and Float32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("Ti", [np.int32, np.int64])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_spmm_split_colmajor_long_rows(hp, orc, gen, T, Ti, k):
    """hpcla_spmm_split_colmajor_{f64,f32}_{i32,i64} (lanes = rows) on the general structure, whose rows of 465 ... 3 000 entries the
    existing special-value test does not have; own block column-major, ghost rows row-major doubles (Float32: the widened
    values, as the exchange delivers them); the long rows' expected classes differ (asserted).  Rule E."""
    vals = gen[_dt(T)]["vals"]
    n, nc, nnz = gen["n"], gen["nc"], len(vals)
    B = sv.operand(nc, k, T)
    want = _oracle_mm(orc, gen["rowptr"], gen["col"], vals, B)
    _long_rows_keep_their_classes(want)
    rp, cv, nz = _t(gen["rowptr"].astype(Ti)), _t(gen["col"].astype(Ti)), _t(vals)
    n_own = 2500
    ldb, ldg, ldc = n_own + 4, k + 2, n + 8
    Bo = _t(_padded(np.ascontiguousarray(B[:n_own].T), ldb))
    Bg = _t(_padded(B[n_own:].astype(np.float64), ldg))
    C = _full((k, ldc), T)
    hp._capi.call(f"hpcla_spmm_split_colmajor_{_dt(T)}_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bo.data_ptr(), ldb, Bg.data_ptr(),
                  ldg, n_own, C.data_ptr(), ldc, n, nnz, k, 0, None, 0, _s())
    got = C.cpu().numpy()
    same(got[:, :n].T, want, f"colmajor {_dt(T)} {_sfx(Ti)} k={k}")
    assert np.all(got[:, n:] == SENT)


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_float32_spmv_and_spmm(hp, orc, gen, Ti):
    """hpcla_spmv_csr_f32_*, hpcla_spmv_split_f32_* (ghosts are doubles holding widened Float32 values: Inf, NaN, -0.0 and a
    Float32 denormal among them, asserted), hpcla_spmm_csr_f32_* in both layouts and hpcla_spmm_split_f32_*, on the general structure with its long
    rows.  Rule E in Float32."""
    T = np.float32
    d = gen["f32"]
    vals, B = d["vals"], d["B"]
    n, nc, nnz = gen["n"], gen["nc"], len(vals)
    want = _oracle_mm(orc, gen["rowptr"], gen["col"], vals, B)
    _long_rows_keep_their_classes(want)
    assert want.dtype == np.float32
    rp, cv, nz = _t(gen["rowptr"].astype(Ti)), _t(gen["col"].astype(Ti)), _t(vals)
    n_own = 2500
    for c in range(4):
        x = B[:, c].copy()
        xd, y = _t(x), _full((n,), T)
        hp._capi.call(f"hpcla_spmv_csr_f32_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xd.data_ptr(), y.data_ptr(), n, nnz, 0, _s())
        same(y.cpu().numpy(), want[:, c], f"f32 csr column {c}")
        x[sv.BAND[1] + 205] = np.finfo(T).tiny / 8            # ghost entries behind the long rows' band
        x[sv.BAND[1] + 200] = [np.nan, np.inf, -0.0, -np.inf][c]
        ghost = x[n_own:].astype(np.float64)
        assert (np.isnan(ghost).any() or np.isinf(ghost).any()) and (ghost == float(np.finfo(T).tiny / 8)).any()
        w2 = _oracle_mv(orc, gen["rowptr"], gen["col"], vals, x)
        xo, xg = _t(x[:n_own]), _t(ghost)
        y.fill_(SENT)
        hp._capi.call(f"hpcla_spmv_split_f32_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), xo.data_ptr(), xg.data_ptr(), n_own,
                      y.data_ptr(), n, nnz, 0, None, 0, _s())
        same(y.cpu().numpy(), w2, f"f32 split column {c}")
    ROW, COL = hp._capi.LAYOUT_ROW, hp._capi.LAYOUT_COL
    Br, Bc = _t(B), _t(np.ascontiguousarray(B.T))
    Cr = _full((n, 4), T)
    hp._capi.call(f"hpcla_spmm_csr_f32_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Br.data_ptr(), 4, ROW, Cr.data_ptr(), 4, ROW,
                  n, nnz, 4, 0, _s())
    same(Cr.cpu().numpy(), want, "f32 row-major SpMM")
    Cc = _full((4, n), T)
    hp._capi.call(f"hpcla_spmm_csr_f32_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bc.data_ptr(), nc, COL, Cc.data_ptr(), n, COL,
                  n, nnz, 4, 0, _s())
    same(Cc.cpu().numpy().T, want, "f32 column-major SpMM")
    Bo, Bg = _t(B[:n_own]), _t(_padded(B[n_own:].astype(np.float64), 6))       # hpcla_spmm_split_f32_*: widened ghost rows
    Cr.fill_(SENT)
    hp._capi.call(f"hpcla_spmm_split_f32_{_sfx(Ti)}", rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), Bo.data_ptr(), 4, Bg.data_ptr(), 6, n_own,
                  Cr.data_ptr(), 4, n, nnz, 4, 0, None, 0, _s())
    same(Cr.cpu().numpy(), want, "f32 split SpMM")


# ---------------------------------------------------------------------------------------------------------------------
# transpose(X) * A and X * A
# ---------------------------------------------------------------------------------------------------------------------
def _dense(hp, backend, M, layout):
    torch = _torch()
    n, w = M.shape
    if layout == "row":
        T = torch.from_numpy(np.ascontiguousarray(M)).cuda()
    else:
        T = torch.from_numpy(np.ascontiguousarray(M.T)).cuda().t()
    return hp.HPCMatrix(hp.uniform_partition(n, 1), hp.uniform_partition(w, 1), T, backend)


@pytest.mark.parametrize("m", [2, 16, 17, 64])
def test_dense_times_sparse(hp, orc, gen, m):
    """transpose(X) @ A and X @ A (csrc/spmm_t.hip) with X row- and column-major.  Expected: the oracle's SpMM over the CSR of
    A^T with equal columns in row order (the order test_bit_identity_with_the_existing_paths pins).  The column present in
    every non-empty row holds > 1 024 entries (asserted), so its sum takes several CHUNK_T passes; its expected class is +Inf,
    -Inf, NaN or finite by the column of X (asserted).  Rule E."""
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    vals = gen["f64"]["vals"]
    n, nc = gen["n"], gen["nc"]
    t_rp, t_row, t_val = sv.transpose_csr(gen["rowptr"], gen["col"], vals, nc)
    assert np.diff(t_rp).max() > 1024
    X = sv.operand(n, m, np.float64, per=12, ordinary=[r for r, _ in sv.ZERO_ROWS])
    want = _oracle_mm(orc, t_rp, t_row, t_val, X).T                   # m x nc
    assert sv.class_of_values(want[:, sv.DENSE_COL]).tolist() == [(sv.PINF, sv.NINF, sv.NAN, sv.FINITE)[c % 4] for c in range(m)]
    A = hp.HPCSparseMatrix_local(gen["rowptr"], gen["col"], vals, nc, backend)
    for layout in ("row", "col"):
        same((hp.transpose(_dense(hp, backend, X, layout)) @ A).gather(), want, f"transpose(X) @ A, X {layout}-major")
        same((_dense(hp, backend, np.ascontiguousarray(X.T), layout) @ A).gather(), want, f"X @ A, X {layout}-major")
    hp.clear_plan_cache()


# ---------------------------------------------------------------------------------------------------------------------
# SpGEMM and sparse A +- B
# ---------------------------------------------------------------------------------------------------------------------
def _csr_of(M):
    return M.rowptr.astype(np.int64), M.col_indices[M.colval.astype(np.int64)], M.nzval.cpu().numpy()


def _small_sparse(rng, nrows, ncols, mean, long_row=None):
    lens = rng.integers(0, 2 * mean, nrows)
    if long_row:
        lens[long_row[0]] = long_row[1]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(ncols, int(l), replace=False)) for l in lens]).astype(np.int64)
    vals = rng.standard_normal(len(col))
    for v in (0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(np.float64).tiny / 8, np.finfo(np.float64).max):
        vals[rng.choice(len(vals), max(2, len(vals) // 60), replace=False)] = v
    return rowptr, col, vals


@pytest.mark.parametrize("which", ["i32", "i64"])
def test_spgemm_special_values(hp, orc, gpu_backend_i32, gpu_backend_i64, which):
    """A @ B through matmat.py three times (first: symbolic + numeric kernels; later products run on the cached structure and,
    once built, on the per-entry product lists of hpcla_spgemm_numeric_mapped_f64 -- asserted) against orc.spgemm: each C(i, j)
    is the first product ASSIGNED, the others added in ascending k, so an entry that is a single -0.0 product stays -0.0 and
    explicit zeros stay stored.  Rule E including the sign of every zero."""
    from hpcla_amd.matmat import clear_matrix_plan_cache, get_matrix_plan
    b = gpu_backend_i32 if which == "i32" else gpu_backend_i64
    rng = np.random.default_rng(21)
    a_rp, a_col, a_val = _small_sparse(rng, 400, 300, 6, long_row=(17, 80))
    b_rp, b_col, b_val = _small_sparse(rng, 300, 200, 5)
    ci = np.unique(a_col)
    cv = np.searchsorted(ci, a_col)
    g_rowptr = np.concatenate([[0], np.cumsum(np.diff(b_rp)[ci])])
    sel = np.concatenate([np.arange(b_rp[r], b_rp[r + 1]) for r in ci])
    with np.errstate(all="ignore"):
        w_rp, w_col, w_val = orc.spgemm(a_rp, cv, a_val, g_rowptr, b_col[sel], b_val[sel], 200)
    assert np.isnan(w_val).any() and np.isinf(w_val).any() and (w_val == 0).any() and (np.signbit(w_val) & (w_val == 0)).any()
    A = hp.HPCSparseMatrix_local(a_rp, a_col, a_val, 300, b)
    B = hp.HPCSparseMatrix_local(b_rp, b_col, b_val, 200, b)
    for rep in range(3):
        rp_c, col_c, val_c = _csr_of(A @ B)
        np.testing.assert_array_equal(rp_c, w_rp)
        np.testing.assert_array_equal(col_c, w_col)
        same(val_c, w_val, f"product {rep + 1}")
    res = get_matrix_plan(A, B).cache["symbolic"]["result"]
    assert res.get("map") is not None, "the product lists were not built"
    clear_matrix_plan_cache()


@pytest.mark.parametrize("Ti", [np.int32, np.int64])
def test_sparse_addition_special_values(hp, gpu_backend_i32, Ti):
    """hpcla_merge_combine_f64_{i32,i64} and A + B / A - B (addition.py): an entry present in one operand is a COPY (a lone
    -0.0 stays -0.0, -(+0.0) is -0.0, never an addition to zero), an entry in both is one + / - -- numpy elementwise.  Rule E."""
    rng = np.random.default_rng(31)
    a_rp, a_col, a_val = _small_sparse(rng, 500, 400, 5)
    b_rp, b_col, b_val = _small_sparse(rng, 500, 400, 5)
    ka = np.repeat(np.arange(500), np.diff(a_rp)) * 400 + a_col
    kb = np.repeat(np.arange(500), np.diff(b_rp)) * 400 + b_col
    keys = np.union1d(ka, kb)
    ia = np.where(np.isin(keys, ka), np.searchsorted(ka, keys), -1)
    ib = np.where(np.isin(keys, kb), np.searchsorted(kb, keys), -1)
    both, only_a, only_b = (ia >= 0) & (ib >= 0), ib < 0, ia < 0
    assert both.sum() > 20 and only_a.sum() > 100 and only_b.sum() > 100
    wants = []
    for sub in (0, 1):
        want = np.empty(len(keys))
        with np.errstate(all="ignore"):
            av, bv = a_val[np.maximum(ia, 0)], b_val[np.maximum(ib, 0)]
            want[both] = (av - bv if sub else av + bv)[both]
            want[only_a] = av[only_a]
            want[only_b] = (-bv if sub else bv)[only_b]
        wants.append(want)
        out = _full((len(keys),), np.float64)
        da, db, dia, dib = _t(a_val), _t(b_val), _t(ia.astype(Ti)), _t(ib.astype(Ti))
        hp._capi.call(f"hpcla_merge_combine_f64_{_sfx(Ti)}", out.data_ptr(), da.data_ptr(), dia.data_ptr(), db.data_ptr(), dib.data_ptr(),
                      len(keys), sub, _s())
        same(out.cpu().numpy(), want, f"merge_combine subtract={sub}")
    assert (np.signbit(wants[1]) & (wants[1] == 0)).any()
    if Ti == np.int32:
        from hpcla_amd.addition import clear_addition_plan_cache
        A = hp.HPCSparseMatrix_local(a_rp, a_col, a_val, 400, gpu_backend_i32)
        B = hp.HPCSparseMatrix_local(b_rp, b_col, b_val, 400, gpu_backend_i32)
        for sub, C in ((0, A + B), (1, A - B)):
            rp_c, col_c, val_c = _csr_of(C)
            np.testing.assert_array_equal(np.repeat(np.arange(500), np.diff(rp_c)) * 400 + col_c, keys)
            same(val_c, wants[sub], f"host layer subtract={sub}")
        clear_addition_plan_cache()


# ---------------------------------------------------------------------------------------------------------------------
# vector updates and the CG kernels
# ---------------------------------------------------------------------------------------------------------------------
def _special_vector(n, T, shift, seed):
    rng = np.random.default_rng(seed)
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, np.finfo(T).tiny / 8, np.finfo(T).max, 1.5], dtype=T)
    x = (rng.random(n) - 0.5).astype(T)
    for i in range(min(n, len(sp))):
        x[i] = sp[(i + shift) % len(sp)]
        x[n - 1 - i] = sp[(i + shift + 3) % len(sp)]
    return x


@pytest.mark.parametrize("n", [1, 2, 513])
def test_vector_updates(hp, gpu_backend_i32, n):
    """axpy, xpay, scale, divide, axpby (f64 and f32 entries), -v and u - v with scalars 0.0, -1.0, Inf, a finite one, and a
    device num / den of 0 / 0; every special value in x and y, at the first elements and at the odd tail.  numpy elementwise
    with separately rounded operations: 0 * Inf is NaN, x / 0.0 is +-Inf, 0.0 / 0.0 is NaN.  Rule E incl. the sign of zero."""
    torch = _torch()
    call = hp._capi.call
    for shift in range(8 if n < 513 else 2):
        x, y = _special_vector(n, np.float64, shift, 1), _special_vector(n, np.float64, shift + 5, 2)
        xd = _t(x)
        zero, one = _t(np.zeros(1)), _t(np.ones(1))
        with np.errstate(all="ignore"):
            for a in (0.0, -1.0, np.inf, 0.37):
                yd = _t(y)
                call("hpcla_axpy_f64", a, None, None, xd.data_ptr(), yd.data_ptr(), n, _s())
                same(yd.cpu().numpy(), y + a * x, f"axpy a={a}")
                yd = _t(y)
                call("hpcla_xpay_f64", xd.data_ptr(), a, None, None, yd.data_ptr(), n, _s())
                same(yd.cpu().numpy(), x + a * y, f"xpay a={a}")
                z = _full((n,), np.float64)
                call("hpcla_scale_f64", a, xd.data_ptr(), z.data_ptr(), n, _s())
                same(z.cpu().numpy(), a * x, f"scale a={a}")
                call("hpcla_divide_f64", xd.data_ptr(), a, z.data_ptr(), n, _s())
                same(z.cpu().numpy(), x / a, f"divide a={a}")
                yd = _t(y)
                call("hpcla_axpby_f64", a, xd.data_ptr(), -1.0, yd.data_ptr(), z.data_ptr(), n, _s())
                same(z.cpu().numpy(), a * x + -1.0 * y, f"axpby a={a}")
            for num, den, s in ((zero, zero, np.nan), (one, zero, np.inf), (zero, one, 0.0)):
                yd = _t(y)
                call("hpcla_axpy_f64", 1.0, num.data_ptr(), den.data_ptr(), xd.data_ptr(), yd.data_ptr(), n, _s())
                same(yd.cpu().numpy(), y + s * x, f"axpy device scalar {s}")
                yd = _t(y)
                call("hpcla_xpay_f64", xd.data_ptr(), 1.0, num.data_ptr(), den.data_ptr(), yd.data_ptr(), n, _s())
                same(yd.cpu().numpy(), x + s * y, f"xpay device scalar {s}")
            u, v = hp.HPCVector.from_global(x, gpu_backend_i32), hp.HPCVector.from_global(y, gpu_backend_i32)
            same((-v).local_values(), -1.0 * y, "-v")
            same((u - v).local_values(), 1.0 * x + -1.0 * y, "u - v")
            # Float32 entries
            F = np.float32
            xf, yf = _special_vector(n, F, shift, 3), _special_vector(n, F, shift + 5, 4)
            pad = np.zeros(4, F)
            xfd, yfd = _t(np.concatenate([xf, pad]))[:n], _t(np.concatenate([yf, pad]))[:n]
            zf = _full((n + 4,), F)
            for a in (F(0.0), F(-1.0), F(np.inf), F(1.7)):
                call("hpcla_axpby_f32", float(a), xfd.data_ptr(), float(F(-0.3)), yfd.data_ptr(), zf.data_ptr(), n, _s())
                same(zf[:n].cpu().numpy(), a * xf + F(-0.3) * yf, f"axpby_f32 a={a}")
                call("hpcla_scale_f32", float(a), xfd.data_ptr(), zf.data_ptr(), n, _s())
                same(zf[:n].cpu().numpy(), a * xf, f"scale_f32 a={a}")
                call("hpcla_divide_f32", xfd.data_ptr(), float(a), zf.data_ptr(), n, _s())
                same(zf[:n].cpu().numpy(), xf / a, f"divide_f32 a={a}")
                assert np.all(zf[n:].cpu().numpy() == SENT)
    del torch


def test_cg_kernels_propagate_poison(hp, orc):
    """hpcla_cg_update_f64, hpcla_cg_residual_f64, hpcla_cg_direction_f64 with one NaN and one Inf in Ap resp. p: the vectors
    under rule E (numpy, separately rounded), the rr scalar under rule C.  hpcla_cg_iterations_f64_i32, 3 iterations on a
    matrix with one NaN value: the call returns and rr_hist[1:] are NaN -- the poison reaches the caller."""
    torch = _torch()
    lib = hp._capi.load()
    n = 1001
    rng = np.random.default_rng(41)
    work = torch.empty(lib.hpcla_reduce_work_bytes() // 8, dtype=torch.float64, device="cuda")
    num, den = _t(np.array([0.75])), _t(np.array([1.5]))
    s = 1.0 * 0.75 / 1.5
    for special, where in ((np.nan, 0), (np.inf, n - 1), (-np.inf, 500), (np.nan, n - 1)):
        p, Ap, x, r = (rng.random(n) - 0.5 for _ in range(4))
        p[where], Ap[(where + 7) % n] = special, special
        with np.errstate(all="ignore"):
            wx, wr = x + s * p, r + (-s) * Ap
            wp = wr + (1.0 * 0.3 / 0.7) * p
        pd, Apd, xd, rd = _t(p), _t(Ap), _t(x), _t(r)
        rr = _full((1,), np.float64)
        hp._capi.call("hpcla_cg_update_f64", None, 1.0, num.data_ptr(), den.data_ptr(), pd.data_ptr(), Apd.data_ptr(), xd.data_ptr(),
                      rd.data_ptr(), n, rr.data_ptr(), work.data_ptr(), _s())
        same(xd.cpu().numpy(), wx, "cg_update x")
        same(rd.cpu().numpy(), wr, "cg_update r")
        with np.errstate(all="ignore"):
            scalar_classed(rr.item(), wr * wr, "cg_update rr")
        assert not math.isfinite(rr.item())
        xd, rd = _t(x), _t(r)
        rr.fill_(SENT)
        hp._capi.call("hpcla_cg_residual_f64", None, 1.0, num.data_ptr(), den.data_ptr(), Apd.data_ptr(), rd.data_ptr(), n, rr.data_ptr(),
                      work.data_ptr(), _s())
        same(rd.cpu().numpy(), wr, "cg_residual r")
        with np.errstate(all="ignore"):
            scalar_classed(rr.item(), wr * wr, "cg_residual rr")
        bnum, bden = _t(np.array([0.3])), _t(np.array([0.7]))
        hp._capi.call("hpcla_cg_direction_f64", 1.0, num.data_ptr(), den.data_ptr(), 1.0, bnum.data_ptr(), bden.data_ptr(), rd.data_ptr(),
                      xd.data_ptr(), pd.data_ptr(), n, _s())
        same(xd.cpu().numpy(), wx, "cg_direction x")
        same(pd.cpu().numpy(), wp, "cg_direction p")
    N = 40
    rows = orc.poisson2d_rows(N, N, 0, N * N)
    vals = rows.vals.copy()
    vals[len(vals) // 2] = np.nan
    nn = N * N
    b = orc.fill_uniform(0, nn, orc.SEED_RHS)
    rp, cv, nz = _t(rows.rowptr.astype(np.int32)), _t(rows.colidx.astype(np.int32)), _t(vals)
    x, r, p, Ap = _t(np.zeros(nn)), _t(b), _t(b), _full((nn,), np.float64)
    hist = _full((4,), np.float64)
    hist[0] = float(np.dot(b, b))
    pAp = _full((1,), np.float64)
    dot_work = torch.empty(lib.hpcla_spmv_dot_work_bytes(nn) // 8 + 1, dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_cg_iterations_f64_i32", None, None, rp.data_ptr(), cv.data_ptr(), nz.data_ptr(), nn, rows.nnz, 0, None, 0, None, 0,
                  x.data_ptr(), r.data_ptr(), p.data_ptr(), Ap.data_ptr(), hist.data_ptr(), pAp.data_ptr(), dot_work.data_ptr(),
                  work.data_ptr(), 3, _s())
    torch.cuda.synchronize()
    h = hist.cpu().numpy()
    assert h[0] == float(np.dot(b, b)) and np.all(np.isnan(h[1:])), h
    assert math.isnan(pAp.item()) and np.isnan(x.cpu().numpy()).any()


# ---------------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 64, 513, 100_003])
def test_reductions(hp, n, T):
    """dot, nrm2sq, asum, amax, sum, prod, powsum (p = 3, 1.5), maxval (both signs) -- the f64 entries and the f32 ones that
    exist -- with one NaN, one +Inf, or +Inf and -Inf, placed at index 0, mid and n - 1 (the odd tail element).  Rule C: the
    class of the scalar from the list of products (amax / maxval: numpy's NaN-propagating max, exactly)."""
    torch = _torch()
    lib = hp._capi.load()
    f64 = np.dtype(T) == np.float64
    t = _dt(T)
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    work = torch.empty(lib.hpcla_reduce_work_bytes() // 8, dtype=torch.float64, device="cuda")

    def red(fn, *args):
        out.fill_(SENT)
        hp._capi.call(fn, None, *args, out.data_ptr(), work.data_ptr(), _s())
        return float(out.item())

    def dev(a):
        return _t(np.concatenate([a, np.zeros(4, a.dtype)]))[:n]

    def eq(a, b):
        return (math.isnan(a) and math.isnan(b)) or a == b

    rng = np.random.default_rng(n)
    y = (rng.random(n) - 0.5).astype(T)
    y[y == 0] = T(0.125)
    yd = dev(y)
    y64 = y.astype(np.float64)
    for where in sorted({0, n // 2, n - 1}):
        for case in ("nan", "pinf", "pinf_ninf"):
            x = sv.vector(n, T, case, where)
            x64 = x.astype(np.float64)
            xd = dev(x)
            tag = f"n={n} {case}@{where}"
            with np.errstate(all="ignore"):
                scalar_classed(red(f"hpcla_dot_{t}", xd.data_ptr(), yd.data_ptr(), n), x64 * y64, f"dot {tag}")
                scalar_classed(red(f"hpcla_nrm2sq_{t}", xd.data_ptr(), n), x64 * x64, f"nrm2sq {tag}")
                scalar_classed(red(f"hpcla_asum_{t}", xd.data_ptr(), n), np.abs(x64), f"asum {tag}")
                scalar_classed(red(f"hpcla_sum_{t}", xd.data_ptr(), n), x64, f"sum {tag}")
                assert eq(red(f"hpcla_amax_{t}", xd.data_ptr(), n), float(np.max(np.abs(x64)))), f"amax {tag}"
                assert eq(red(f"hpcla_maxval_{t}", xd.data_ptr(), n, 0), float(np.max(x64))), f"maxval {tag}"
                assert eq(red(f"hpcla_maxval_{t}", xd.data_ptr(), n, 1), float(np.max(-x64))), f"maxval(-x) {tag}"
                if not f64:
                    continue
                for pw in (3.0, 1.5):
                    scalar_classed(red("hpcla_powsum_f64", xd.data_ptr(), n, pw), np.abs(x64) ** pw, f"powsum {pw} {tag}")
                # prod: factors 1 + x / 1000 > 0; NaN -> NaN, one Inf -> the product's sign, 0 and Inf -> NaN in any order
                f = 1.0 + 1e-3 * np.where(np.isfinite(x64), x64, 0.0)
                f[~np.isfinite(x64)] = x64[~np.isfinite(x64)]
                fd = _t(f)
                got = red("hpcla_prod_f64", fd.data_ptr(), n)
                want = np.nan if case == "nan" else (np.inf if case == "pinf" or n == 1 else -np.inf)
                assert eq(got, want), f"prod {tag}: {got}"
                if n > 1:
                    f[(where + 1) % n] = 0.0
                    fd = _t(f)
                    got = red("hpcla_prod_f64", fd.data_ptr(), n)
                    assert math.isnan(got), f"prod with 0 and Inf {tag}: {got}"


@pytest.mark.parametrize("case", ["nan", "pinf", "pinf_ninf"])
def test_reductions_host_layer(hp, gpu_backend_i32, case):
    """hp.norm(v) (p = 2, 1, Inf, 3), hp.dot, hp.vsum, hp.prod, hp.maximum / minimum on a poisoned vector: what a caller of
    the host layer sees.  Rule C."""
    n = 513
    for where in (0, 256, n - 1):
        x = sv.vector(n, np.float64, case, where)
        y = np.random.default_rng(5).random(n) + 0.25
        v, w = hp.HPCVector.from_global(x, gpu_backend_i32), hp.HPCVector.from_global(y, gpu_backend_i32)
        with np.errstate(all="ignore"):
            scalar_classed(hp.dot(v, w), x * y, "dot")
            scalar_classed(hp.vsum(v), x, "vsum")
            scalar_classed(hp.norm(v) ** 2, x * x, "norm 2")
            scalar_classed(hp.norm(v, 1), np.abs(x), "norm 1")
            scalar_classed(hp.norm(v, 3) ** 3, np.abs(x) ** 3, "norm 3")
            for got, want in ((hp.norm(v, math.inf), np.max(np.abs(x))), (hp.maximum(v), np.max(x)), (hp.minimum(v), np.min(x))):
                assert (math.isnan(got) and math.isnan(want)) or got == want
            got = hp.prod(hp.HPCVector.from_global(np.where(np.isfinite(x), 1.0 + 1e-3 * x, x), gpu_backend_i32))
            want = {"nan": np.nan, "pinf": np.inf, "pinf_ninf": -np.inf}[case]
            assert (math.isnan(got) and math.isnan(want)) or got == want


# ---------------------------------------------------------------------------------------------------------------------
# gram and dense A * x / A' x
# ---------------------------------------------------------------------------------------------------------------------
def _block(M, layout, pad):
    n, w = M.shape
    if layout == "row":
        buf = np.full((n, w + pad), SENT, dtype=M.dtype)
        buf[:, :w] = M
        return _t(buf), w + pad
    buf = np.full((w, n + pad), SENT, dtype=M.dtype)
    buf[:, :n] = M.T
    return _t(buf), n + pad


def _gram_operand(n, w, T, seed):
    """Columns c % 4 == 0: one +Inf, 2: one NaN, 3: -0.0 and a denormal, 1: ordinary -- so that the classes of the cells of
    X'Y differ (finite, +-Inf, NaN) at every width."""
    rng = np.random.default_rng(seed)
    M = (rng.random((n, w)) - 0.5).astype(T)
    for c in range(w):
        r = rng.integers(1, n - 1, 3)
        if c % 4 == 0:                                       # at the first / the last row: the edges of the row chunks
            M[0 if c % 8 == 0 else n - 1, c] = np.inf if c % 8 == 0 else -np.inf
        elif c % 4 == 2:
            M[r[0], c] = np.nan
        elif c % 4 == 3:
            M[r[0], c], M[r[1], c] = -0.0, np.finfo(T).tiny / 8
    return M


@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("xl,yl", [("row", "row"), ("row", "col"), ("col", "row"), ("col", "col")])
def test_gram(hp, T, xl, yl):
    """hpcla_gram_{f64,f32}, four layout pairs, widths 3, 16, 17, a row count that is no multiple of the chunk: out-of-range rows
    are padded with zeros inside the kernel -- 0 * Inf would be a NaN in a cell whose class is Inf.  Rule C per cell; X == Y
    stays exactly symmetric, NaN positions included."""
    torch = _torch()
    from hpcla_amd.vectors import current_stream_ptr, dptr
    lay = {"row": hp._capi.LAYOUT_ROW, "col": hp._capi.LAYOUT_COL}
    n = 3001
    f64 = np.dtype(T) == np.float64

    def gram(X, Y, same_block):
        m, k = X.shape[1], Y.shape[1]
        Xd, ldx = _block(X, xl, 1)
        Yd, ldy = (Xd, ldx) if same_block else _block(Y, yl, 2)
        C = _full((m, k), np.float64)
        work = torch.empty(max(1, hp._capi.load().hpcla_gram_work_bytes(n, m, k) // 8), dtype=torch.float64, device="cuda")
        hp._capi.call(f"hpcla_gram_{_dt(T)}", None, dptr(Xd), ldx, lay[xl], dptr(Yd), ldy, lay[xl if same_block else yl], n, m, k,
                      dptr(C), dptr(work), current_stream_ptr())
        return C.cpu().numpy()

    def check(got, X, Y, what):
        with np.errstate(all="ignore"):
            P = X.astype(np.float64)[:, :, None] * Y.astype(np.float64)[:, None, :]
        cls = sv.classes_of(P, axis=0)
        assert (cls == sv.FINITE).any() and (cls == sv.NAN).any() and ((cls == sv.PINF) | (cls == sv.NINF)).any()
        fin = np.where(np.isfinite(P), P, 0.0)
        exact = np.array([[math.fsum(fin[:, i, j]) for j in range(P.shape[2])] for i in range(P.shape[1])])
        if f64:
            classed(got, cls, exact, np.abs(fin).sum(axis=0), what)
        else:
            assert np.array_equal(sv.class_of_values(got), cls), what
            f = cls == sv.FINITE
            w32 = exact.astype(np.float32)
            assert np.all(np.abs(got.astype(np.float32).astype(np.float64)[f] - w32.astype(np.float64)[f])
                          <= np.spacing(np.abs(w32)).astype(np.float64)[f]), what

    for m, k in ((3, 16), (16, 17), (17, 3)):
        X, Y = _gram_operand(n, m, T, 50 + m), _gram_operand(n, k, T, 70 + k)
        check(gram(X, Y, False), X, Y, f"gram {m} x {k}")
    for m in (3, 16, 17):
        X = _gram_operand(n, m, T, 90 + m)
        S = gram(X, X, True)
        check(S, X, X, f"X'X width {m}")
        assert np.array_equal(S, S.T, equal_nan=True), "X'X not exactly symmetric"


@pytest.mark.parametrize("shape", [(5000, 16), (257, 64), (40, 700)])
def test_dense_matvec_and_transpose_matvec(hp, gpu_backend_i32, shape):
    """dense_matvec (A @ x, csrc/gemv.hip incl. gemv_skinny, which pads x with 0.0 and starts from the first product) and
    dense_matvec_t (transpose(A) @ x): specials in A alone (most outputs finite), then in x as well (x = +-Inf turns 0 * x
    padding into NaN where the class is Inf).  Rule C: class per output, 1e-12 * sum |a||x| on the finite ones; the sign of an
    exact zero is not asserted."""
    b = gpu_backend_i32
    m, n = shape
    rng = np.random.default_rng(m + n)
    A = rng.random((m, n)) - 0.5
    for v in (np.inf, -np.inf, np.nan, -0.0, 0.0, np.finfo(np.float64).tiny / 8):
        A[rng.integers(0, m, 4), rng.integers(0, n, 4)] = v
    A[0, 0], A[m - 1, n - 1] = np.inf, -np.inf
    Ad = hp.HPCMatrix.from_global(A, b)
    for special_x in (False, True):
        x, xt = rng.random(n) - 0.5, rng.random(m) - 0.5
        x[n // 3], xt[m // 3] = -0.0, -0.0
        if special_x:
            x[0], x[n - 1], xt[0], xt[m - 1] = np.inf, -np.inf, -np.inf, np.inf
            A2 = A.copy()
            A2[1, 0], A2[0, 1], A2[m - 1, 2], A2[2, n - 1] = 0.0, 0.0, 0.0, 0.0       # 0 * Inf in both products
            Ad, Ah = hp.HPCMatrix.from_global(A2, b), A2
        else:
            Ah = A
        with np.errstate(all="ignore"):
            P = Ah * x[None, :]
            Pt = Ah * xt[:, None]
        for got, prod, axis, what in (((Ad @ hp.HPCVector.from_global(x, b)).local_values(), P, 1, "A @ x"),
                                      ((hp.transpose(Ad) @ hp.HPCVector.from_global(xt, b)).local_values(), Pt, 0, "A' @ x")):
            cls = sv.classes_of(prod, axis=axis)
            fin = np.where(np.isfinite(prod), prod, 0.0)
            classed(got, cls, fin.sum(axis=axis), np.abs(fin).sum(axis=axis) + 1e-300, f"{what} {shape} special x = {special_x}")
            if not special_x:
                assert (cls == sv.FINITE).any() and (cls != sv.FINITE).any()
            else:                                                # every output holds an Inf product: the classes still differ
                assert (cls == sv.NAN).any() and (cls == sv.PINF).any() and (cls == sv.NINF).any()
    hp.clear_dense_plan_cache()
