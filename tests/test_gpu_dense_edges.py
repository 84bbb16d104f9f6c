"""The dense kernels of csrc/gemv.hip (A*x, transpose(A)*x) and the layout conversion hpcla_transpose_f64/_f32 of
csrc/spmm.hip where they branch: every lane-group width of the skinny kernel on, one below and one above a wavefront's rows;
odd and padded pitches; A, the work area and the x segments off their 16-byte alignment (the ghost-buffer form of the
distributed A*x among them); the eight-way unrolled loops of both transpose(A)*x stages, which need many chunks or many rows
at a narrow width; few rows and very many columns (the orientation the Julia extension calls with); the narrow and the generic
conversion kernel on padded leading dimensions, from offset sources and as strided block copies -- through the raw C ABI.

References and cases come from tests/_dense_edge_cases.py (checked on the CPU by tests/test_dense_edge_cases.py).
Integer-valued inputs are compared for equality with the int64 product, whatever the summation order; real-valued ones with a
long-double sum within RTOL_RED * sum|a||x|; x = e_j must give column j (row i for the transpose) exactly.

Every output -- y, the work area, the conversion's destination -- lies inside a larger tensor of NaN with at least GUARD
elements on either side, and whatever the call must not write is NaN afterwards: an overrun lands in memory the test owns and
fails an assertion.  Padding of every input is NaN too, and no NaN may reach an output."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dense_edge_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

G = dc.GUARD
NAN = float("nan")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _nan_buffer(n, off=0, dtype=None):
    """(tensor of G + off + n + G NaN elements, address of its element G + off): the n elements a call may write.  The tensor
    starts on a 16-byte boundary (asserted), so the interior does exactly when `off` is even."""
    import torch
    buf = torch.full((G + off + n + G,), NAN, dtype=dtype or torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0 and (G * buf.element_size()) % 16 == 0
    return buf, buf.data_ptr() + (G + off) * buf.element_size()


def _interior(buf, n, off=0, what=""):
    """The n interior elements of a _nan_buffer on the host, after asserting that both guards are still NaN."""
    got = buf.cpu().numpy()
    assert np.isnan(got[:G + off]).all(), f"{what}: written before the output"
    assert np.isnan(got[G + off + n:]).all(), f"{what}: written past the output"
    return got[G + off:G + off + n]


def _place_A(A_dev, lda, a_off):
    """A (nrows x ncols, contiguous, on the device) on pitch lda inside a NaN buffer, starting a_off elements past a 16-byte
    boundary; the padding columns stay NaN.  Returns (buffer, address of A[0, 0])."""
    nrows, ncols = A_dev.shape
    buf, ptr = _nan_buffer(nrows * lda, a_off)
    buf[G + a_off:G + a_off + nrows * lda].view(nrows, lda)[:, :ncols] = A_dev
    assert (ptr % 16 == 0) == (a_off % 2 == 0)
    return buf, ptr


def _assert_product(got, kind, want, scale, what):
    assert not np.isnan(got).any(), f"{what}: NaN in the output (padding was read, or an element was not written)"
    if kind == "int":
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        err = np.abs(got - want)
        worst = int(np.argmax(err - dc.RTOL_RED * scale))
        assert np.all(err <= dc.RTOL_RED * scale), f"{what}: output {worst} off by {err[worst]:.3e}, sum|a||x| {scale[worst]:.3e}"


# ---- transpose(A) * x -------------------------------------------------------------------------------------------------

def _gemv_t(hp, Aptr, lda, nrows, ncols, x_dev, w_off, d, reps):
    """`reps` calls into the rows of one NaN matrix and ONE work area; returns the outputs (reps x ncols)."""
    import torch
    nwork = d["work_bytes"] // 8
    wbuf, wptr = _nan_buffer(nwork, w_off)
    ybuf = torch.full((reps, G + ncols + G), NAN, dtype=torch.float64, device="cuda")
    for r in range(reps):
        hp._capi.call("hpcla_gemv_t_rowmajor_f64", Aptr, lda, nrows, ncols, x_dev.data_ptr(), ybuf[r].data_ptr() + 8 * G, wptr,
                      _stream())
    torch.cuda.synchronize()
    y = ybuf.cpu().numpy()
    assert np.isnan(y[:, :G]).all() and np.isnan(y[:, G + ncols:]).all(), "written outside y_full"
    work = _interior(wbuf, nwork, w_off, "work")
    assert not np.isnan(work).any(), "a partial sum of the work area was not written, or holds NaN"
    return y[:, G:G + ncols]


def _gemv_t_probes(hp, Aptr, lda, nrows, ncols, w_off, d, rows):
    """x = e_i for every i of `rows`; returns the outputs (len(rows) x ncols)."""
    import torch
    nwork = d["work_bytes"] // 8
    wbuf, wptr = _nan_buffer(nwork, w_off)
    x = torch.zeros(nrows, dtype=torch.float64, device="cuda")
    ybuf = torch.full((len(rows), G + ncols + G), NAN, dtype=torch.float64, device="cuda")
    for r, i in enumerate(rows.tolist()):
        x[i:i + 1].fill_(1.0)
        hp._capi.call("hpcla_gemv_t_rowmajor_f64", Aptr, lda, nrows, ncols, x.data_ptr(), ybuf[r].data_ptr() + 8 * G, wptr,
                      _stream())
        x[i:i + 1].fill_(0.0)
    torch.cuda.synchronize()
    y = ybuf.cpu().numpy()
    assert np.isnan(y[:, :G]).all() and np.isnan(y[:, G + ncols:]).all(), "written outside y_full"
    _interior(wbuf, nwork, w_off, "work")
    return y[:, G:G + ncols]


@pytest.mark.parametrize("group", list(dc.GEMVT_GROUPS))
def test_gemv_t(hp, group):
    """Every shape of the group in its four forms (own pitch, pitch + 1, A 8 bytes off, work area 8 bytes off), integer- and
    real-valued, each called twice (same bits); and x = e_i at both sides of every chunk edge returns row i."""
    forms = [c for c in dc.gemv_t_cases() if c[0] == group]
    assert forms
    for nrows, ncols, _ in dc.GEMVT_GROUPS[group]:
        mine = [c for c in forms if c[1:3] == (nrows, ncols)]
        for kind in ("int", "real"):
            A, x = dc.product_inputs(kind, nrows, ncols, nrows, 11)
            want, scale = (dc.ref_int(A, x, True), None) if kind == "int" else dc.ref_longdouble(A, x, True)
            A_dev, x_dev = _dev(A), _dev(x)
            for _, _, _, form, lda, a_off, w_off, d in mine:
                what = f"{nrows} x {ncols} {form} (lda {lda}, {d['kernel']}, {d['nchunks']} chunks) {kind}"
                Abuf, Aptr = _place_A(A_dev, lda, a_off)
                y = _gemv_t(hp, Aptr, lda, nrows, ncols, x_dev, w_off, d, reps=2)
                _assert_product(y[0], kind, want, scale, what)
                np.testing.assert_array_equal(y[0].view(np.uint64), y[1].view(np.uint64), err_msg=f"{what}: second call")
                if kind == "real":
                    rows = dc.gemv_t_probe_rows(nrows, ncols, every=(form == "plain"))
                    got = _gemv_t_probes(hp, Aptr, lda, nrows, ncols, w_off, d, rows)
                    bad = np.flatnonzero((got != A[rows]).any(axis=1))
                    assert len(bad) == 0, f"{what}: x = e_i does not return row i for i in {rows[bad[:8]].tolist()}"
                del Abuf


# ---- A * x ------------------------------------------------------------------------------------------------------------

def _segments(xfull, split, xform):
    """(x_lo, x_own, x_hi addresses, tensors to keep alive) of the device vector xfull cut as `split`: "separate" gives every
    segment a tensor of its own, "ghost" puts the lower and the higher one into ONE buffer, x_hi = ghost + 8 * n_lo."""
    import torch
    n_lo, n_own, n_hi = split
    own = xfull[n_lo:n_lo + n_own].clone() if n_own else None
    p_own = own.data_ptr() if n_own else None
    if xform == "ghost":
        ghost = torch.cat([xfull[:n_lo], xfull[n_lo + n_own:]]).clone() if n_lo + n_hi else None
        p_lo = ghost.data_ptr() if n_lo else None
        p_hi = ghost.data_ptr() + 8 * n_lo if n_hi else None
        keep = (own, ghost)
    else:
        lo = xfull[:n_lo].clone() if n_lo else None
        hi = xfull[n_lo + n_own:].clone() if n_hi else None
        p_lo, p_hi = lo.data_ptr() if n_lo else None, hi.data_ptr() if n_hi else None
        keep = (own, lo, hi)
    for t in keep:
        assert t is None or t.data_ptr() % 16 == 0
    return p_lo, p_own, p_hi, keep


def _gemv_block(hp, Aptr, lda, nrows, xfull, picks):
    """One call per (split, x form) of `picks` on the same A, into the rows of one NaN matrix; returns len(picks) x nrows."""
    import torch
    ybuf = torch.full((len(picks), G + nrows + G), NAN, dtype=torch.float64, device="cuda")
    alive = []
    for r, (_, split, xform) in enumerate(picks):
        p_lo, p_own, p_hi, keep = _segments(xfull, split, xform)
        alive.append(keep)
        hp._capi.call("hpcla_gemv_rowmajor_f64", Aptr, lda, nrows, p_lo, split[0], p_own, split[1], p_hi, split[2],
                      ybuf[r].data_ptr() + 8 * G, _stream())
    torch.cuda.synchronize()
    y = ybuf.cpu().numpy()
    assert np.isnan(y[:, :G]).all() and np.isnan(y[:, G + nrows:]).all(), "written outside y"
    return y[:, G:G + nrows]


@pytest.mark.parametrize("group", dc.GEMV_GROUPS)
def test_gemv(hp, group):
    """Every shape of the group (one lane-group width of the skinny kernel at its wavefront edges, or the row-per-wavefront
    kernel) on pitches ncols + {0, 1, 2, 7}, A on and 8 bytes off a 16-byte boundary, x cut into three segments that are
    tensors of their own or share a ghost buffer; integer- and real-valued."""
    cases = dc.gemv_cases(group)
    inputs = {}
    for nrows, ncols, lda, a_off, picks in cases:
        if (nrows, ncols) not in inputs:
            entry = {}
            for kind in ("int", "real"):
                A, x = dc.product_inputs(kind, nrows, ncols, ncols, 13)
                want, scale = (dc.ref_int(A, x, False), None) if kind == "int" else dc.ref_longdouble(A, x, False)
                entry[kind] = (_dev(A), _dev(x), want, scale)
            inputs = {(nrows, ncols): entry}                   # the shapes come in runs: keep the current one only
        for kind in ("int", "real"):
            A_dev, x_dev, want, scale = inputs[(nrows, ncols)][kind]
            Abuf, Aptr = _place_A(A_dev, lda, a_off)
            y = _gemv_block(hp, Aptr, lda, nrows, x_dev, picks)
            for r, (name, split, xform) in enumerate(picks):
                _assert_product(y[r], kind, want, scale, f"{nrows} x {ncols} lda {lda} A+{8 * a_off} {name} {split} {xform} {kind}")
            del Abuf


def test_gemv_every_width_1_to_130(hp):
    """37 rows of every width from 1 to 130 (both kernels, every lane-group width at every column count it serves), integer
    inputs, on the exact and on an odd-making pitch, x whole and cut at odd places inside a ghost buffer."""
    nrows = dc.SWEEP_NROWS
    for ncols in dc.SWEEP_NCOLS:
        A, x = dc.product_inputs("int", nrows, ncols, ncols, 17)
        want = dc.ref_int(A, x, False)
        A_dev, x_dev = _dev(A), _dev(x)
        splits = dc.segment_splits(ncols)
        name = "odd_odd_rest" if "odd_odd_rest" in splits else "all_own"
        picks = [("all_own", splits["all_own"], "separate"), (name, splits[name], "ghost")]
        for lda in (ncols, ncols + 1):
            Abuf, Aptr = _place_A(A_dev, lda, 0)
            y = _gemv_block(hp, Aptr, lda, nrows, x_dev, picks)
            for r in range(len(picks)):
                _assert_product(y[r], "int", want, None, f"37 x {ncols} lda {lda} {picks[r][0]}")
            del Abuf


def test_gemv_one_hot_returns_the_column(hp):
    """x = e_j returns column j of a real-valued A exactly, for j on both sides of every segment edge and j = ncols - 1, at
    every width of the case tables, on an even and an odd pitch, with separate segments and a ghost buffer."""
    import torch
    for ncols in dc.SKINNY_NCOLS + dc.ROWMAJOR_NCOLS:
        nrows = dc.rows_per_wave(ncols) + 1 if ncols <= dc.SKINNY_MAX else 5
        A, _ = dc.product_inputs("real", nrows, ncols, ncols, 19)
        A_dev = _dev(A)
        splits = dc.segment_splits(ncols)
        split = splits["odd_odd_rest"] if "odd_odd_rest" in splits else splits["all_own"]
        probes = sorted(set(dc.segment_edges(split)) | {ncols - 1})
        for lda in (ncols, ncols + 1):
            Abuf, Aptr = _place_A(A_dev, lda, 0)
            for xform in dc.X_FORMS:
                for j in probes:
                    x = torch.zeros(ncols, dtype=torch.float64, device="cuda")
                    x[j] = 1.0
                    y = _gemv_block(hp, Aptr, lda, nrows, x, [("", split, xform)])[0]
                    assert np.all(y == A[:, j]), f"{nrows} x {ncols} lda {lda} {split} {xform}: x = e_{j} is not column {j}"
            del Abuf


# ---- layout conversion ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("group", dc.TRANSPOSE_GROUPS)
def test_transpose(hp, group, dtype):
    """The destination buffer, guards and padding included, equals numpy's: the matrix where the layout says, NaN everywhere
    else -- for the generic 32 x 32 tile kernel (all four layout pairs, sizes around the tile), the narrow 256-row kernel
    (sizes around its workgroup, padded sources; a padded destination leaves it) and the argument forms of the Julia
    extension (padded operand rows, an oddly offset source, block placement as a strided ROW -> ROW copy)."""
    import torch
    sfx, tdtype = ("f64", torch.float64) if dtype == np.float64 else ("f32", torch.float32)
    es = np.dtype(dtype).itemsize
    for c in dc.transpose_cases(group):
        src, want = dc.transpose_buffers(c, dtype)
        dsrc = _dev(src)
        dst = torch.full((len(want),), NAN, dtype=tdtype, device="cuda")
        hp._capi.call(f"hpcla_transpose_{sfx}", dsrc.data_ptr() + c["src_off"] * es, c["ld_src"], c["src_layout"],
                      dst.data_ptr() + (G + c["dst_off"]) * es, c["ld_dst"], c["dst_layout"], c["rows"], c["cols"], _stream())
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"{c['name']} ({c['kernel']} kernel, {sfx})")   # NaN equals NaN here


# ---- empty operands and refused arguments -----------------------------------------------------------------------------

def test_degenerate_sizes(hp):
    import torch
    call, s = hp._capi.call, _stream()
    vals = torch.arange(1, 65, dtype=torch.float64, device="cuda")
    p = vals.data_ptr()
    # A*x without rows: nothing is written
    ybuf, yptr = _nan_buffer(8)
    call("hpcla_gemv_rowmajor_f64", p, 4, 0, None, 0, p, 4, None, 0, yptr, s)
    call("hpcla_gemv_rowmajor_f64", None, 0, 0, None, 0, None, 0, None, 0, None, s)
    torch.cuda.synchronize()
    assert np.isnan(ybuf.cpu().numpy()).all()
    # A*x without columns: every y[i] is +0.0, A may be null
    for nrows in (1, 5, 300):
        ybuf, yptr = _nan_buffer(nrows)
        call("hpcla_gemv_rowmajor_f64", None, 0, nrows, None, 0, None, 0, None, 0, yptr, s)
        torch.cuda.synchronize()
        assert np.all(_interior(ybuf, nrows, 0, f"{nrows} x 0").view(np.uint64) == 0)
    # transpose(A)*x without rows: zeros over the NaN, nothing else is needed
    for ncols in (1, 5, 1000):
        ybuf, yptr = _nan_buffer(ncols)
        call("hpcla_gemv_t_rowmajor_f64", None, ncols, 0, ncols, None, yptr, None, s)
        torch.cuda.synchronize()
        assert np.all(_interior(ybuf, ncols, 0, f"0 x {ncols}").view(np.uint64) == 0)
    # ... and without columns: nothing to write
    call("hpcla_gemv_t_rowmajor_f64", None, 0, 5, 0, None, None, None, s)
    call("hpcla_gemv_t_rowmajor_f64", p, 0, 5, 0, p, None, None, s)
    # conversions of nothing
    for sfx, dt in (("f64", torch.float64), ("f32", torch.float32)):
        dbuf, dptr = _nan_buffer(16, dtype=dt)
        for rows, cols in ((0, 4), (4, 0), (0, 0)):
            for sl, dl in dc.LAYOUT_PAIRS:
                call(f"hpcla_transpose_{sfx}", p, 4, sl, dptr, 4, dl, rows, cols, s)
                call(f"hpcla_transpose_{sfx}", None, 4, sl, None, 4, dl, rows, cols, s)
        torch.cuda.synchronize()
        assert np.isnan(dbuf.cpu().numpy()).all()
    assert np.array_equal(vals.cpu().numpy(), np.arange(1.0, 65.0))


def test_argument_errors(hp):
    """Bad arguments come back as a status (HPCLAError) and nothing is launched: the outputs keep their NaN."""
    import torch
    call, s = hp._capi.call, _stream()
    HPCLAError = hp._capi.HPCLAError
    vals = torch.arange(1, 65, dtype=torch.float64, device="cuda")
    p = vals.data_ptr()
    ybuf, y = _nan_buffer(32)
    wbuf, w = _nan_buffer(32)

    def gemv(A=p, lda=4, nrows=2, x_lo=None, n_lo=0, x_own=p, n_own=4, x_hi=None, n_hi=0, out=y):
        call("hpcla_gemv_rowmajor_f64", A, lda, nrows, x_lo, n_lo, x_own, n_own, x_hi, n_hi, out, s)

    def gemv_t(A=p, lda=4, nrows=2, ncols=4, x=p, out=y, work=w):
        call("hpcla_gemv_t_rowmajor_f64", A, lda, nrows, ncols, x, out, work, s)

    def transpose(sfx, src=p, ld_src=4, sl=dc.LAYOUT_ROW, dst=y, ld_dst=4, dl=dc.LAYOUT_ROW, rows=2, cols=4):
        call(f"hpcla_transpose_{sfx}", src, ld_src, sl, dst, ld_dst, dl, rows, cols, s)

    gemv()                                                           # the defaults themselves are valid calls
    gemv_t()
    transpose("f64")
    torch.cuda.synchronize()
    ybuf.fill_(NAN)
    wbuf.fill_(NAN)
    for bad in (dict(lda=3), dict(nrows=-1), dict(n_own=-1, x_own=None), dict(n_lo=-1), dict(n_hi=-1),
                dict(n_lo=1, x_lo=p, n_hi=1, x_hi=p, lda=5)):        # 6 columns on a pitch of 5
        with pytest.raises(HPCLAError, match="bad sizes"):
            gemv(**bad)
    for bad in (dict(out=None), dict(A=None)):
        with pytest.raises(HPCLAError, match="null pointer"):
            gemv(**bad)
    for bad in (dict(x_own=None), dict(n_lo=1, lda=5), dict(n_hi=2, lda=6)):
        with pytest.raises(HPCLAError, match="null x segment"):
            gemv(**bad)
    for bad in (dict(lda=3), dict(nrows=-1), dict(ncols=-1)):
        with pytest.raises(HPCLAError, match="bad sizes"):
            gemv_t(**bad)
    with pytest.raises(HPCLAError, match="null output"):
        gemv_t(out=None)
    with pytest.raises(HPCLAError, match="null output"):
        gemv_t(out=None, nrows=0)
    for bad in (dict(work=None), dict(A=None), dict(x=None)):
        with pytest.raises(HPCLAError, match="null pointer"):
            gemv_t(**bad)
    for sfx in ("f64", "f32"):
        for bad in (dict(rows=-1), dict(cols=-1)):
            with pytest.raises(HPCLAError, match="negative"):
                transpose(sfx, **bad)
        for bad in (dict(src=None), dict(dst=None)):
            with pytest.raises(HPCLAError, match="null pointer"):
                transpose(sfx, **bad)
        for bad in (dict(sl=2), dict(sl=-1), dict(dl=2), dict(dl=-1), dict(sl=7, dl=7)):
            with pytest.raises(HPCLAError, match="layout"):
                transpose(sfx, **bad)
        # one column more than the generic kernel's grid holds: refused before the launch (the pointers are never followed)
        too_many = 65535 * 32 + 1
        for sl, dl, ld_src, ld_dst in ((dc.LAYOUT_ROW, dc.LAYOUT_COL, too_many, 1), (dc.LAYOUT_COL, dc.LAYOUT_ROW, 1, too_many),
                                       (dc.LAYOUT_ROW, dc.LAYOUT_ROW, too_many, too_many)):
            with pytest.raises(HPCLAError, match="more than"):
                transpose(sfx, ld_src=ld_src, sl=sl, ld_dst=ld_dst, dl=dl, rows=1, cols=too_many)
    torch.cuda.synchronize()
    assert np.isnan(ybuf.cpu().numpy()).all() and np.isnan(wbuf.cpu().numpy()).all()
    assert np.array_equal(vals.cpu().numpy(), np.arange(1.0, 65.0))


# ---- host layer -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,wide,c0", [(1027, 16, 23, 3), (301, 200, 211, 5), (14401, 32, 33, 1)])
def test_host_layer_takes_a_column_slice_as_local_block(hp, gpu_backend_i32, m, n, wide, c0):
    """An HPCMatrix whose local block is a non-contiguous view (columns c0 .. c0+n-1 of a wider tensor): A @ x and
    transpose(A) @ x give the bits of the contiguous copy, and those are right."""
    b = gpu_backend_i32
    rng = np.random.default_rng(m)
    Wg, xg, xtg = rng.random((m, wide)) - 0.5, rng.random(n) - 0.5, rng.random(m) - 0.5
    Ag = np.ascontiguousarray(Wg[:, c0:c0 + n])
    Mc = hp.HPCMatrix.from_global(Ag, b)
    view = _dev(Wg)[:, c0:c0 + n]
    assert not view.is_contiguous() and Mc.A.is_contiguous()
    Mv = hp.HPCMatrix(Mc.row_partition, Mc.col_partition, view, b)
    x, xt = hp.HPCVector.from_global(xg, b), hp.HPCVector.from_global(xtg, b)
    for transposed, v, vg in ((False, x, xg), (True, xt, xtg)):
        got_v = ((hp.transpose(Mv) if transposed else Mv) @ v).local_values()
        got_c = ((hp.transpose(Mc) if transposed else Mc) @ v).local_values()
        np.testing.assert_array_equal(got_v.view(np.uint64), got_c.view(np.uint64))
        want, scale = dc.ref_longdouble(Ag, vg, transposed)
        _assert_product(got_v, "real", want, scale, f"{m} x {n} view, transposed {transposed}")
    np.testing.assert_array_equal(view.cpu().numpy(), Ag)              # the view itself was not written
    hp.clear_dense_plan_cache()
