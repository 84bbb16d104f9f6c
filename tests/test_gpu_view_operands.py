"""Every host-layer operation on operands that are VIEWS of a caller's buffer (tests/_view_operands.py): 8 bytes (Float32: 4, 8 or
12) off a 16-byte boundary, on odd and even pitches, column ranges, column-major.  The constructors keep such a tensor as it is;
the vector kernels of the C ABI work in 16-byte accesses and refuse a pointer off that boundary (a documented status, asserted by
the raw-ABI tests).  The host layer passes such a vector operand as a clone, or computes into aligned scratch and copies back
(vectors.rd16 / wr16); the matrix kernels that have an 8-byte form take the view where it is.

Every cell is (operation, operand position, variant): each position alone over all variants, then all positions off "fresh"
together.  Before every call the operand's ``data_ptr() % 16`` is asserted to be what the variant's name says (torch's allocator
returns 512-byte aligned blocks: without the check the sweep could silently test aligned operands).  After every call: the NaN
poison around every operand is untouched, read-only operands keep their bits, and an operand the operation writes holds the
result IN THE CALLER'S BUFFER (one bit-compare of the whole buffer against its expected image).  Results are compared with
references that are never the device's own: numpy's separately rounded expression (bit-equal), ``math.fsum`` (sums, within
1e-12 of the sum of |terms|), the oracle's sequential products (bit-equal), and for the solvers the true residual from the
gathered result within the bound of the solver's own convergence test -- plus bit-equality with the same solve on fresh clones,
which holds because both runs put the same values through the same kernels.

Single rank, the default stream.  No skips: every cell runs."""
import functools
import math

import numpy as np
import pytest

from tests import _bicgstab_cases as bc
from tests import _dense_edge_cases as dec
from tests import _eigsh_cases as ec
from tests import _grid_regimes as gr
from tests import _lobpcg_cases as lbc
from tests import _lsqr_cases as lc
from tests import _minres_cases as mc
from tests import _pcg_cases as pc
from tests import _qr_cases as qc
from tests import _svds_cases as sc
from tests import _view_operands as vo

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
RTOL_RED = dec.RTOL_RED                                          # 1e-12, relative to the sum of |terms|
assert RTOL_RED == lbc.RED_RTOL == 1e-12
# the smallest sizes at which a double2 body plus a scalar tail can go wrong, one past the first stage-1 workgroup (2051: two
# partials), and R3_N: 301 partials in Float64, 150 in Float32, 1201 elementwise workgroups
VEC_N = (1, 2, 3, 257, 2051, gr.R3_N)
assert gr.reduce_grid(2051) == 2 and gr.reduce_grid(gr.R3_N) > 1 and gr.f32_reduce_grid(gr.R3_N) > 1
MAT_N, MAT_K = (1, 65, 257), (1, 2, 3, 8, 16, 17)
MAT_NK = [(n, k) for n in MAT_N for k in MAT_K]
BACKENDS = ("i32", "i64", "f32")
F64_BACKENDS = ("i32", "i64")


@pytest.fixture(scope="module")
def backends(hp, gpu_backend_i32, gpu_backend_i64):
    yield {"i32": gpu_backend_i32, "i64": gpu_backend_i64, "f32": hp.backend_rocm_serial(np.float32, np.int32)}
    _MATRICES.clear()
    hp.clear_plan_cache()
    hp.clear_spmm_cache()
    hp.clear_dense_plan_cache()


def _dtype(which):
    return F32 if which == "f32" else F64


def _vvars(which):
    return vo.vector_variants(_dtype(which))


def _ids(c):
    return "-".join(c)


# ---- placing operands and checking them afterwards --------------------------------------------------------------------------------
class Placed:
    """Values inside a poisoned device buffer: the buffer, the operand view, a snapshot of the whole buffer."""

    def __init__(self, values, variant, matrix=False):
        self.variant, self.matrix, self.shape = variant, matrix, values.shape
        place = vo.place_matrix if matrix else vo.place_vector
        self.buf, self.t = place(values, variant, device="cuda")
        promise = (vo.matrix_promise(variant, *values.shape, values.dtype) if matrix else vo.vector_promise(variant, values.dtype))
        assert (self.t.data_ptr() % 16, self.t.is_contiguous()) == promise, (variant, self.t.data_ptr() % 16)
        self.promise = promise
        self.snap = self.buf.clone()

    def image(self, values):
        """The whole buffer as it must look when the operand holds ``values`` and nothing else changed."""
        import torch
        img = self.snap.clone()
        view = vo.matrix_view(img, self.variant, *self.shape) if self.matrix else vo.vector_view(img, self.variant, self.shape[0])
        view.copy_(torch.from_numpy(np.array(values)))
        return img

    def unchanged(self):
        import torch
        assert torch.equal(vo.bits(self.buf), vo.bits(self.snap)), f"{self.variant}: a read-only operand or its poison changed"

    def holds(self, values):
        import torch
        assert torch.equal(vo.bits(self.buf), vo.bits(self.image(values))), \
            f"{self.variant}: the caller's buffer does not hold the result (or the poison around it changed)"


def _hvec(hp, backend, placed):
    """The HPCVector around the view; asserts that the pointer the C ABI will see is the view's and as misaligned as promised."""
    v = hp.HPCVector_local(placed.t, backend)
    assert v.v.data_ptr() == placed.t.data_ptr() and v.v.data_ptr() % 16 == placed.promise[0], placed.variant
    return v


def _hmat(hp, backend, placed):
    """The HPCMatrix around the view: ``HPCMatrix_local`` for a contiguous block (it keeps a tensor that already fits), the
    constructor for the strided ones (``HPCMatrix_local`` would pack them); the same pointer and pitch assertion."""
    n, k = placed.shape
    if placed.variant in ("fresh", "off8"):
        M = hp.HPCMatrix_local(placed.t, backend)
        assert M.shape == (n, k)
    else:
        M = hp.HPCMatrix(np.array([0, n], dtype=np.int64), np.array([0, k], dtype=np.int64), placed.t, backend)
    assert M.A.data_ptr() == placed.t.data_ptr() and M.A.data_ptr() % 16 == placed.promise[0], placed.variant
    assert M.A.stride() == placed.t.stride()
    return M


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    it = np.int32 if got.dtype == F32 else np.int64
    assert np.array_equal(got.view(it), want.view(it)), f"{what}: {int((got.view(it) != want.view(it)).sum())} values differ in a bit"


def _same_info(info, other, what):
    """Every field of a solver's info dataclass: floats, lists and arrays of floats bit for bit (history and anorm included),
    everything else equal."""
    import dataclasses
    assert type(info) is type(other)
    for f in dataclasses.fields(info):
        a, b = getattr(info, f.name), getattr(other, f.name)
        if isinstance(a, (float, list, tuple, np.ndarray)):
            _same_bits(np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1), f"{what} info.{f.name}")
        else:
            assert a == b, (what, f.name, a, b)


# ---- values and references, computed once --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _values(n, dtype, seed, lo=-1.0, hi=1.0):
    v = np.random.default_rng(1000 * seed + n % 997).uniform(lo, hi, n).astype(dtype)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _block(n, k, dtype, seed, integer=False):
    rng = np.random.default_rng(7919 * seed + 31 * n + k)
    v = (rng.integers(-3, 4, (n, k)).astype(dtype) if integer else rng.uniform(-1.0, 1.0, (n, k)).astype(dtype))
    v.setflags(write=False)
    return v


_FSUMS = {}


def _fsum_terms(terms, key=None):
    """(math.fsum of the terms, of their magnitudes); with a ``key`` that names the terms, computed once."""
    if key is not None and key in _FSUMS:
        return _FSUMS[key]
    terms = np.asarray(terms, dtype=np.float64)
    out = math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist())
    if key is not None:
        _FSUMS[key] = out
    return out


POW_ULPS = 2 * float(np.finfo(np.float64).eps)                   # |x|^p on the device and in numpy: each within one ulp of the term


def _within_margin(got, terms, dtype, post=None, what="", key=None, term_rtol=0.0, post_ulps=0):
    """``got`` against math.fsum of the (double) terms within RTOL_RED of the sum of |terms|.  A Float32 backend rounds the
    double result once to Float32 (and ``post``, the square root, before that): rounding is monotone, so the result lies between
    the roundings of the two ends of the margin.  ``term_rtol``: how far the device's terms themselves may be from the
    reference's (a pow: POW_ULPS), relative to each |term|.  ``post_ulps``: a ``post`` that is not correctly rounded (the host's
    ``** (1 / 3)``, within one ulp on either side) moves each end of the window outwards by that many ulps."""
    s, sabs = _fsum_terms(terms, key)
    lo, hi = s - (RTOL_RED + term_rtol) * sabs, s + (RTOL_RED + term_rtol) * sabs
    if post is not None:
        lo, hi = post(max(lo, 0.0)), post(hi)
        for _ in range(post_ulps):
            lo, hi = float(np.nextafter(lo, -np.inf)), float(np.nextafter(hi, np.inf))
    if dtype == F32:
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
    print(f"{what}: got {got!r}, fsum window [{lo!r}, {hi!r}]")
    assert lo <= got <= hi, (what, got, lo, hi)


A_SCALE, A_DIV = 2.5, 3.0                                        # exact in both element types


# ---- 1. element-wise: new vectors ------------------------------------------------------------------------------------------------------
def _tr(hp):
    return hp.transpose


BINARY = {
    "u+v": (lambda hp, u, v: u + v, lambda U, V: U + V),
    "u-v": (lambda hp, u, v: u - v, lambda U, V: U - V),
    "u'+v'": (lambda hp, u, v: (_tr(hp)(u) + _tr(hp)(v)).parent, lambda U, V: U + V),
    "u'-v'": (lambda hp, u, v: (_tr(hp)(u) - _tr(hp)(v)).parent, lambda U, V: U - V),
}
UNARY = {
    "-v": (lambda hp, v: -v, lambda V: V.dtype.type(-1.0) * V),
    "a*v": (lambda hp, v: A_SCALE * v, lambda V: V.dtype.type(A_SCALE) * V),
    "v*a": (lambda hp, v: v * A_SCALE, lambda V: V.dtype.type(A_SCALE) * V),
    "v/a": (lambda hp, v: v / A_DIV, lambda V: V / V.dtype.type(A_DIV)),
    "-v'": (lambda hp, v: (-_tr(hp)(v)).parent, lambda V: V.dtype.type(-1.0) * V),
    "a*v'": (lambda hp, v: (A_SCALE * _tr(hp)(v)).parent, lambda V: V.dtype.type(A_SCALE) * V),
    "v'*a": (lambda hp, v: (_tr(hp)(v) * A_SCALE).parent, lambda V: V.dtype.type(A_SCALE) * V),
    "v'/a": (lambda hp, v: (_tr(hp)(v) / A_DIV).parent, lambda V: V / V.dtype.type(A_DIV)),
}


@pytest.mark.parametrize("which", BACKENDS)
@pytest.mark.parametrize("op", sorted(BINARY))
def test_binary_elementwise(hp, backends, which, op):
    B, dt = backends[which], _dtype(which)
    run, ref = BINARY[op]
    for n in VEC_N:
        U, V = _values(n, dt, 1), _values(n, dt, 2)
        want = ref(U, V)
        assert want.dtype == dt
        for cu, cv in vo.combos(_vvars(which), _vvars(which)):
            pu, pv = Placed(U, cu), Placed(V, cv)
            out = run(hp, _hvec(hp, B, pu), _hvec(hp, B, pv))
            _same_bits(out.local_values(), want, f"{op} n={n} {cu},{cv}")
            assert out.v.data_ptr() not in (pu.t.data_ptr(), pv.t.data_ptr())
            pu.unchanged(), pv.unchanged()


@pytest.mark.parametrize("which", BACKENDS)
@pytest.mark.parametrize("op", sorted(UNARY))
def test_unary_elementwise(hp, backends, which, op):
    B, dt = backends[which], _dtype(which)
    run, ref = UNARY[op]
    for n in VEC_N:
        V = _values(n, dt, 3)
        want = ref(V)
        assert want.dtype == dt
        for (cv,) in vo.combos(_vvars(which)):
            pv = Placed(V, cv)
            out = run(hp, _hvec(hp, B, pv))
            _same_bits(out.local_values(), want, f"{op} n={n} {cv}")
            pv.unchanged()


# ---- 2. element-wise: in place (Float64 entries) ------------------------------------------------------------------------------------------
A_UPD = 0.75


@pytest.mark.parametrize("which", F64_BACKENDS)
@pytest.mark.parametrize("op", ["axpy_", "xpay_"])
def test_inplace_updates_land_in_the_callers_buffer(hp, backends, which, op):
    B = backends[which]
    for n in VEC_N:
        Y, X = _values(n, F64, 4), _values(n, F64, 5)
        want = Y + A_UPD * X if op == "axpy_" else X + A_UPD * Y
        for cy, cx in vo.combos(vo.VECTOR_F64, vo.VECTOR_F64):
            py, px = Placed(Y, cy), Placed(X, cx)
            y, x = _hvec(hp, B, py), _hvec(hp, B, px)
            back = y.axpy_(A_UPD, x) if op == "axpy_" else y.xpay_(x, A_UPD)
            assert back is y and y.v.data_ptr() == py.t.data_ptr()
            py.holds(want), px.unchanged()


def _scalars():
    import torch
    num = torch.tensor([0.7], dtype=torch.float64, device="cuda")
    den = torch.tensor([1.3], dtype=torch.float64, device="cuda")
    return num, den, np.float64(2.0) * np.float64(0.7) / np.float64(1.3)       # dev_scalar: (alpha * num) / den


def _sum_in_margin(got, terms, what, key):
    _within_margin(float(got), terms, F64, what=what, key=key)


@pytest.mark.parametrize("which", F64_BACKENDS)
@pytest.mark.parametrize("combo", vo.combos(*[vo.VECTOR_F64] * 4), ids=_ids)
def test_cg_update_lands_in_the_callers_buffers(hp, backends, which, combo):
    """x += s p; r -= s Ap; rr = sum r^2 with s = a num / den from device scalars: positions (x, r, p, Ap)."""
    import torch
    B = backends[which]
    num, den, s = _scalars()
    for n in VEC_N:
        X, R, P, Q = (_values(n, F64, 6 + i) for i in range(4))
        px, pr, pp, pq = (Placed(v, c) for v, c in zip((X, R, P, Q), combo))
        rr = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        hp.cg_update_(*(_hvec(hp, B, p) for p in (px, pr, pp, pq)), 2.0, num, den, rr)
        r_new = R - s * Q
        px.holds(X + s * P), pr.holds(r_new), pp.unchanged(), pq.unchanged()
        _sum_in_margin(rr.item(), r_new * r_new, f"cg_update_ rr n={n} {combo}", ("cg_update_", n))


@pytest.mark.parametrize("which", F64_BACKENDS)
@pytest.mark.parametrize("combo", vo.combos(*[vo.VECTOR_F64] * 2), ids=_ids)
def test_cg_residual_lands_in_the_callers_buffer(hp, backends, which, combo):
    """r -= s Ap; rr = sum r^2: positions (r, Ap)."""
    import torch
    B = backends[which]
    num, den, s = _scalars()
    for n in VEC_N:
        R, Q = _values(n, F64, 10), _values(n, F64, 11)
        pr, pq = Placed(R, combo[0]), Placed(Q, combo[1])
        rr = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        hp.cg_residual_(_hvec(hp, B, pr), _hvec(hp, B, pq), 2.0, num, den, rr)
        r_new = R - s * Q
        pr.holds(r_new), pq.unchanged()
        _sum_in_margin(rr.item(), r_new * r_new, f"cg_residual_ rr n={n} {combo}", ("cg_residual_", n))


@pytest.mark.parametrize("which", F64_BACKENDS)
@pytest.mark.parametrize("combo", vo.combos(*[vo.VECTOR_F64] * 3), ids=_ids)
def test_cg_direction_lands_in_the_callers_buffers(hp, backends, which, combo):
    """x += s p; p = r + t p: positions (x, p, r)."""
    B = backends[which]
    num, den, s = _scalars()
    t = np.float64(0.5) * np.float64(1.3) / np.float64(0.7)
    for n in VEC_N:
        X, P, R = (_values(n, F64, 12 + i) for i in range(3))
        px, pp, pr = (Placed(v, c) for v, c in zip((X, P, R), combo))
        hp.cg_direction_(*(_hvec(hp, B, p) for p in (px, pp, pr)), 2.0, num, den, 0.5, den, num)
        px.holds(X + s * P), pp.holds(R + t * P), pr.unchanged()


# ---- 3. reductions -----------------------------------------------------------------------------------------------------------------------
def _d(v):
    return v.astype(np.float64)


SUMS = {       # name: (Float32 too, run, the double terms, what follows the sum)
    "norm1": (True, lambda hp, v: hp.norm(v, 1), lambda V: np.abs(_d(V)), None),
    "norm2": (True, lambda hp, v: hp.norm(v, 2), lambda V: _d(V) * _d(V), math.sqrt),
    "norm3": (False, lambda hp, v: hp.norm(v, 3), lambda V: np.abs(V) ** 3.0, lambda s: s ** (1.0 / 3.0)),     # a Float64 entry
    "vsum": (True, lambda hp, v: hp.vsum(v), lambda V: _d(V), None),
}


@pytest.mark.parametrize("which,op", [(w, op) for w in BACKENDS for op in sorted(SUMS) if SUMS[op][0] or w != "f32"])
def test_sums_of_one_vector(hp, backends, which, op):
    B, dt = backends[which], _dtype(which)
    _, run, terms, post = SUMS[op]
    for n in VEC_N:
        V = _values(n, dt, 20)
        for (cv,) in vo.combos(_vvars(which)):
            pv = Placed(V, cv)
            got = run(hp, _hvec(hp, B, pv))
            pv.unchanged()
            if op == "norm3":
                # the same window as norm2's: the power sum within RTOL_RED (plus the pow's last place per term) of fsum, its
                # two ends through the cube root, one ulp each way for the two host roots (got's and the end's)
                _within_margin(got, terms(V), dt, post, f"{op} n={n} {cv}", key=(op, n, dt.name), term_rtol=POW_ULPS, post_ulps=2)
            else:
                _within_margin(got, terms(V), dt, post, f"{op} n={n} {cv}", key=(op, n, dt.name))


@pytest.mark.parametrize("which", BACKENDS)
def test_dot(hp, backends, which):
    B, dt = backends[which], _dtype(which)
    for n in VEC_N:
        X, Y = _values(n, dt, 21), _values(n, dt, 22)
        for cx, cy in vo.combos(_vvars(which), _vvars(which)):
            px, py = Placed(X, cx), Placed(Y, cy)
            x, y = _hvec(hp, B, px), _hvec(hp, B, py)
            _within_margin(hp.dot(x, y), _d(X) * _d(Y), dt, None, f"dot n={n} {cx},{cy}", key=("dot", n, dt.name))
            got_row = hp.transpose(x) @ y                        # the row-vector form of the same product
            _within_margin(got_row, _d(X) * _d(Y), dt, None, f"x' * y n={n} {cx},{cy}", key=("dot", n, dt.name))
            px.unchanged(), py.unchanged()
        for (cx,) in vo.combos(_vvars(which)):                   # one vector in both positions
            px = Placed(X, cx)
            x = _hvec(hp, B, px)
            _within_margin(hp.dot(x, x), _d(X) * _d(X), dt, None, f"dot(x, x) n={n} {cx}", key=("dotxx", n, dt.name))
            px.unchanged()


@pytest.mark.parametrize("which", BACKENDS)
@pytest.mark.parametrize("op", ["maximum", "minimum", "norminf"])
def test_exact_reductions(hp, backends, which, op):
    B, dt = backends[which], _dtype(which)
    for n in VEC_N:
        V = _values(n, dt, 23)
        want = {"maximum": float(V.max()), "minimum": float(V.min()), "norminf": float(np.abs(V).max())}[op]
        for (cv,) in vo.combos(_vvars(which)):
            pv = Placed(V, cv)
            v = _hvec(hp, B, pv)
            got = hp.norm(v, math.inf) if op == "norminf" else getattr(hp, op)(v)
            assert got == want, (op, n, cv, got, want)
            pv.unchanged()


@pytest.mark.parametrize("which", F64_BACKENDS)
def test_prod(hp, backends, which):
    """Values exp(u), u uniform in [-0.095, 0.095]: inside [0.9, 1.1] with a log that is symmetric about 0, so the product of
    614 403 of them stays near exp(+-43) (uniform values in [0.9, 1.1] have a mean log of -0.0017 and underflow at that size).
    Reference: the sequential product in extended precision (64-bit significand: at most n 2^-64 = 3.4e-14 relative at the
    largest size, far inside the 1e-12 margin)."""
    B = backends[which]
    assert np.finfo(np.longdouble).nmant >= 63
    for n in VEC_N:
        V = np.exp(_values(n, F64, 24, -0.095, 0.095))
        assert 0.9 <= V.min() and V.max() <= 1.1
        want = float(np.prod(V.astype(np.longdouble)))
        assert math.isfinite(want) and want > 0
        for (cv,) in vo.combos(vo.VECTOR_F64):
            pv = Placed(V, cv)
            got = hp.prod(_hvec(hp, B, pv))
            print(f"prod n={n} {cv}: got {got!r}, want {want!r}")
            assert abs(got - want) <= 1e-12 * want, (n, cv, got, want)
            pv.unchanged()


@pytest.mark.parametrize("which", BACKENDS)
def test_out_arguments_of_the_reductions(hp, backends, which):
    """``out=``, every form that takes one: a 1-element view 8 bytes off inside a poisoned buffer receives the all-reduced
    double -- for p = 2 the sum of squares and for p = 3 the sum of |x|^3 (the root is the caller's), for p = Inf the maximum
    magnitude (one term: exact)."""
    import torch
    B, dt = backends[which], _dtype(which)
    for n in VEC_N:
        X, Y = _values(n, dt, 25), _values(n, dt, 26)
        big = np.zeros(1)
        big[0] = np.abs(_d(X)).max()
        calls = {"dot": (lambda x, y, o: hp.dot(x, y, out=o), _d(X) * _d(Y), 0.0),
                 "norm2": (lambda x, y, o: hp.norm(x, 2, out=o), _d(X) * _d(X), 0.0),
                 "norm1": (lambda x, y, o: hp.norm(x, 1, out=o), np.abs(_d(X)), 0.0),
                 "norminf": (lambda x, y, o: hp.norm(x, math.inf, out=o), big, 0.0),
                 "vsum": (lambda x, y, o: hp.vsum(x, out=o), _d(X), 0.0)}
        if dt == F64:                                            # the power sum is a Float64 entry
            calls["norm3"] = (lambda x, y, o: hp.norm(x, 3, out=o), np.abs(X) ** 3.0, POW_ULPS)
        for name, (run, terms, term_rtol) in calls.items():
            for cx, cy in vo.combos(_vvars(which), _vvars(which)):
                px, py = Placed(X, cx), Placed(Y, cy)
                obuf = torch.full((4,), float("nan"), dtype=torch.float64, device="cuda")
                out = obuf[1:2]
                assert out.data_ptr() % 16 == 8
                back = run(_hvec(hp, B, px), _hvec(hp, B, py), out)
                assert back is out
                host = obuf.cpu().numpy()
                assert np.isnan(host[[0, 2, 3]]).all()
                if name == "norminf":
                    assert float(host[1]) == float(big[0]), (n, cx, cy, host[1], big[0])
                else:
                    _within_margin(float(host[1]), terms, F64, None, f"{name}(out=) n={n} {cx},{cy}", key=("out", name, n, dt.name),
                                   term_rtol=term_rtol)
                px.unchanged(), py.unchanged()


# ---- 4. HPCMatrix * a, / a, norm -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", BACKENDS)
@pytest.mark.parametrize("variant", vo.MATRIX)
def test_dense_scaling_and_norms(hp, backends, which, variant):
    B, dt = backends[which], _dtype(which)
    for n, k in MAT_NK:
        V = _block(n, k, dt, 30)
        pm = Placed(V, variant, matrix=True)
        M = _hmat(hp, B, pm)
        for name, got, want in (("M*a", M * A_SCALE, dt.type(A_SCALE) * V), ("a*M", A_SCALE * M, dt.type(A_SCALE) * V),
                                ("M/a", M / A_DIV, V / dt.type(A_DIV))):
            assert got.A.shape == (n, k)
            _same_bits(got.local_values(), want, f"{name} {n}x{k} {variant}")
        flat = _d(V).reshape(-1)
        _within_margin(M.norm(1), np.abs(flat), dt, None, f"norm(M, 1) {n}x{k} {variant}")
        _within_margin(M.norm(2), flat * flat, dt, math.sqrt, f"norm(M, 2) {n}x{k} {variant}")
        assert M.norm(math.inf) == float(np.abs(V).max())
        pm.unchanged()


# ---- 5. sparse products ------------------------------------------------------------------------------------------------------------------
OFFSETS = (-5, -1, 0, 1, 7)
_MATRICES = {}


@functools.lru_cache(maxsize=None)
def _banded(nrows, ncols, seed, integer=False):
    """CSR (int64) of a banded nrows x ncols matrix: diagonals OFFSETS clipped to the shape, ascending columns, every column of a
    square one stored (so the compressed column space is the whole one)."""
    rows = np.repeat(np.arange(nrows, dtype=np.int64), len(OFFSETS))
    cols = rows + np.tile(np.array(OFFSETS, dtype=np.int64), nrows)
    keep = (cols >= 0) & (cols < ncols)
    rows, cols = rows[keep], cols[keep]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrows))]).astype(np.int64)
    rng = np.random.default_rng(seed + nrows)
    vals = rng.integers(-3, 4, len(cols)).astype(np.float64) if integer else rng.uniform(-1.0, 1.0, len(cols))
    return rowptr, cols, vals


def _sparse(hp, backends, which, nrows, ncols, seed=40, integer=False):
    key = (which, nrows, ncols, seed, integer)
    if key not in _MATRICES:
        rowptr, cols, vals = _banded(nrows, ncols, seed, integer)
        _MATRICES[key] = hp.HPCSparseMatrix_local(rowptr, cols, vals.astype(_dtype(which)), ncols, backends[which])
    return _MATRICES[key]


def _orc_product(orc, which, csr, X):
    """The oracle's sequential product of the CSR with the columns of X (a vector or a block), in the backend's types."""
    rowptr, cols, vals = csr
    it = np.int64 if which == "i64" else np.int32
    dt = _dtype(which)
    args = (rowptr.astype(it), cols.astype(it), vals.astype(dt))
    if X.ndim == 1:
        return orc.spmv(*args, np.ascontiguousarray(X))
    return np.stack([orc.spmv(*args, np.ascontiguousarray(X[:, j])) for j in range(X.shape[1])], axis=1)


@pytest.mark.parametrize("which", BACKENDS)
def test_spmv_reads_a_view_and_writes_into_one(hp, orc, backends, which):
    B, dt = backends[which], _dtype(which)
    for n in VEC_N:
        A = _sparse(hp, backends, which, n, n)
        X = _values(n, dt, 41)
        want = _orc_product(orc, which, _banded(n, n, 40), X)
        for (cx,) in vo.combos(_vvars(which)):
            px = Placed(X, cx)
            y = A @ _hvec(hp, B, px)
            _same_bits(y.local_values(), want, f"A @ x n={n} {cx}")
            px.unchanged()
        for cy, cx in vo.combos(_vvars(which), _vvars(which)):   # mul!(y, A, x): y is the caller's
            py, px = Placed(_values(n, dt, 42), cy), Placed(X, cx)
            y = _hvec(hp, B, py)
            assert hp.mul_(y, A, _hvec(hp, B, px)) is y
            py.holds(want), px.unchanged()


@pytest.mark.parametrize("which", F64_BACKENDS)
def test_transposed_spmv_reads_a_view(hp, orc, backends, which):
    B = backends[which]
    for n in VEC_N:
        A = _sparse(hp, backends, which, n, n)
        rowptr, cols, vals = _banded(n, n, 40)
        X = _values(n, F64, 43)
        want = _orc_product(orc, which, lc.transpose_csr(rowptr, cols, vals, n), X)
        for (cx,) in vo.combos(vo.VECTOR_F64):
            px = Placed(X, cx)
            x = _hvec(hp, B, px)
            y = hp.transpose(A) @ x
            _same_bits(y.local_values(), want, f"transpose(A) @ x n={n} {cx}")
            yt = hp.transpose(x) @ A                             # the row-vector form
            _same_bits(yt.parent.local_values(), want, f"x' @ A n={n} {cx}")
            px.unchanged()


SPMM_KERNELS = ("hpcla_spmm_csr_", "hpcla_spmm_split_", "hpcla_spmm_runs_k16_")       # B is their fourth argument


def _read_in_place(t, pitch):
    """Whether the SpMM promises to read the block where it is: its rows are packed and the kernels' row pitch is k (any 8-byte
    offset: the generic kernels have an 8-byte form), or its rows already sit on the kernels' pitch at a 16-byte aligned base
    (an odd k >= 3 in Float64 runs on pitch k + 1).  Every other block costs one packing copy."""
    k = t.shape[1]
    if pitch == k:
        return t.is_contiguous()
    return t.stride() == (pitch, 1) and t.data_ptr() % 16 == 0


@pytest.mark.parametrize("which", BACKENDS)
@pytest.mark.parametrize("variant", vo.MATRIX)
def test_spmm_on_block_views(hp, orc, backends, which, variant, monkeypatch):
    """A @ B for every block variant, bit-equal per column to the oracle; and the pointer the SpMM kernels are GIVEN for B
    (recorded at the binding) is the caller's view wherever no copy is promised -- a contiguous block 8 bytes off included."""
    spmm_pitch = hp.spmm_plans.spmm_pitch
    B, dt = backends[which], _dtype(which)
    given = []
    real_call = hp._capi.call

    def recording_call(fn_name, *args):
        if fn_name.startswith(SPMM_KERNELS):
            given.append((fn_name, args[3].value))
        return real_call(fn_name, *args)
    monkeypatch.setattr(hp._capi, "call", recording_call)
    in_place = 0
    for n, k in MAT_NK:
        A = _sparse(hp, backends, which, n, n)
        V = _block(n, k, dt, 44)
        want = _orc_product(orc, which, _banded(n, n, 40), V)
        pm = Placed(V, variant, matrix=True)
        M = _hmat(hp, B, pm)
        for name, product in (("A @ B", lambda: A @ M), ("hp.spmm", lambda: hp.spmm(A, M))):
            del given[:]
            C = product()
            assert C.A.shape == (n, k)
            _same_bits(C.local_values(), want, f"{name} {n}x{k} {variant}")
            assert given, "no SpMM kernel was launched through the binding"
            if _read_in_place(pm.t, spmm_pitch(A, k)):
                in_place += 1
                assert all(ptr == pm.t.data_ptr() for _, ptr in given), (name, n, k, variant, given, pm.t.data_ptr())
        pm.unchanged()
    assert in_place, variant                                     # every variant has such cells (n = 1, k = 1, or the pitch that fits)


# ---- 6. dense products -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", F64_BACKENDS)
@pytest.mark.parametrize("combo", vo.combos(vo.MATRIX, vo.VECTOR_F64, vo.VECTOR_F64), ids=_ids)
def test_dense_matvec(hp, backends, which, combo):
    """M @ x and mul!(y, M, x) within the bound of test_dense_transpose_matvec's family: 1e-12 |M| |x|.  Positions (M, x, y): y,
    the caller's result vector, is varied like the other two."""
    B = backends[which]
    cm, cx, cy = combo
    for n, k in MAT_NK:
        Mv, X = _block(n, k, F64, 50), _values(k, F64, 51)
        want, scale = Mv @ X, np.abs(Mv) @ np.abs(X) + 1e-300
        pm, px = Placed(Mv, cm, matrix=True), Placed(X, cx)
        y = _hmat(hp, B, pm) @ _hvec(hp, B, px)
        assert np.all(np.abs(y.local_values() - want) <= 1e-12 * scale), (n, k, combo)
        py = Placed(_values(n, F64, 52), cy)                     # the result into the caller's view
        yv = _hvec(hp, B, py)
        assert hp.dense_matvec(_hmat(hp, B, pm), _hvec(hp, B, px), yv) is yv
        got = py.t.cpu().numpy()
        assert np.all(np.abs(got - want) <= 1e-12 * scale), (n, k, combo)
        py.holds(got)                                            # nothing but the operand changed
        pm.unchanged(), px.unchanged()


@pytest.mark.parametrize("which", F64_BACKENDS)
@pytest.mark.parametrize("combo", vo.combos(vo.MATRIX, vo.VECTOR_F64), ids=_ids)
def test_dense_transposed_matvec(hp, backends, which, combo):
    """transpose(M) @ x and x' @ M within the bound of test_dense_transpose_matvec: 1e-12 |M|' |x|."""
    B = backends[which]
    cm, cx = combo
    for n, k in MAT_NK:
        Mv, X = _block(n, k, F64, 53), _values(n, F64, 54)
        want, scale = Mv.T @ X, np.abs(Mv).T @ np.abs(X) + 1e-300
        pm, px = Placed(Mv, cm, matrix=True), Placed(X, cx)
        M, x = _hmat(hp, B, pm), _hvec(hp, B, px)
        y = hp.transpose(M) @ x
        assert np.all(np.abs(y.local_values() - want) <= 1e-12 * scale), (n, k, combo)
        yt = hp.transpose(x) @ M
        _same_bits(yt.parent.local_values(), y.local_values(), f"x' @ M {n}x{k} {combo}")       # same kernels: same bits
        pm.unchanged(), px.unchanged()


@pytest.mark.parametrize("which", F64_BACKENDS)
@pytest.mark.parametrize("combo", vo.combos(vo.MATRIX, vo.MATRIX), ids=_ids)
def test_gram_of_block_views(hp, backends, which, combo):
    """transpose(X) @ Y on integer-valued blocks: every partial sum is an integer below 2^53, so any order gives numpy's bits."""
    B = backends[which]
    for n, k in MAT_NK:
        Xv, Yv = _block(n, k, F64, 55, integer=True), _block(n, 3, F64, 56, integer=True)
        px, py = Placed(Xv, combo[0], matrix=True), Placed(Yv, combo[1], matrix=True)
        X, Y = _hmat(hp, B, px), _hmat(hp, B, py)
        _same_bits((hp.transpose(X) @ Y).gather(), Xv.T @ Yv, f"X'Y {n}x{k} {combo}")
        _same_bits((hp.transpose(X) @ X).gather(), Xv.T @ Xv, f"X'X {n}x{k} {combo[0]}")
        px.unchanged(), py.unchanged()


@pytest.mark.parametrize("which", F64_BACKENDS)
@pytest.mark.parametrize("variant", vo.MATRIX)
def test_dense_times_sparse_on_block_views(hp, backends, which, variant):
    """transpose(X) @ A and X @ A for an integer-valued X view and an integer-valued sparse A: bit-equal to numpy."""
    B = backends[which]
    for n, k in MAT_NK:
        Xv = _block(n, k, F64, 57, integer=True)
        px = Placed(Xv, variant, matrix=True)
        X = _hmat(hp, B, px)
        A = _sparse(hp, backends, which, n, n + 2, seed=58, integer=True)
        Ad = lc.dense_of(*_banded(n, n + 2, 58, True), n + 2)
        _same_bits((hp.transpose(X) @ A).gather(), Xv.T @ Ad, f"X'A {n}x{k} {variant}")
        A2 = _sparse(hp, backends, which, k, k + 2, seed=59, integer=True)
        A2d = lc.dense_of(*_banded(k, k + 2, 59, True), k + 2)
        _same_bits((X @ A2).gather(), Xv @ A2d, f"XA {n}x{k} {variant}")
        px.unchanged()


# ---- 7. QR and least squares ----------------------------------------------------------------------------------------------------------------
QR_NK = [(1, 1)] + [(n, k) for n in (65, 257) for k in MAT_K]


@pytest.mark.parametrize("variant", vo.MATRIX)
def test_qr_of_a_block_view(hp, backends, variant):
    B = backends["i32"]
    for n, k in QR_NK:
        Xv = qc.make(n, k, 1e3, 60 + k)
        px = Placed(Xv, variant, matrix=True)
        Q, R = hp.qr(_hmat(hp, B, px))
        qc.check_r_shape(R, k)
        q = Q.gather()
        orth, back = qc.orth(q), qc.back(q, R, Xv)
        print(f"qr {n}x{k} {variant}: orth {orth:.1e}, back {back:.1e}, limit {qc.limit(k):.1e}")
        assert orth <= qc.limit(k) and back <= qc.limit(k), (n, k, variant, orth, back)
        Rr = hp.qr(_hmat(hp, B, px), mode="r")
        _same_bits(Rr, R, f"qr mode r {n}x{k} {variant}")
        px.unchanged()


@pytest.mark.parametrize("combo", vo.combos(vo.MATRIX, vo.VECTOR_F64), ids=_ids)
def test_lstsq_of_a_block_view_and_a_vector_view(hp, backends, combo):
    B = backends["i32"]
    for n, k in QR_NK[1:]:
        Xv = qc.make(n, k, 1e3, 70 + k)
        bv = _values(n, F64, 71)
        px, pb = Placed(Xv, combo[0], matrix=True), Placed(bv, combo[1])
        c, rnorm = hp.lstsq(_hmat(hp, B, px), _hvec(hp, B, pb))
        cv = c.gather()
        neq = qc.neq(Xv, bv, cv)
        want = np.linalg.lstsq(Xv, bv, rcond=None)[0]
        assert qc.neq(Xv, bv, want) <= qc.limit(k)               # numpy within the same limit: the generator cannot hide a failure
        print(f"lstsq {n}x{k} {combo}: neq {neq:.1e}, limit {qc.limit(k):.1e}")
        assert neq <= qc.limit(k), (n, k, combo, neq)
        assert math.isfinite(rnorm) and rnorm >= 0.0
        px.unchanged(), pb.unchanged()


# ---- 8. the solvers: b, x0 / the start vector or block and the weights as views --------------------------------------------------------
def _vec_or_none(hp, B, values, variant):
    if values is None:
        return None, None
    p = Placed(values, variant)
    return p, _hvec(hp, B, p)


def _csr_matrix(hp, B, rowptr, colidx, vals, ncols=None):
    return hp.HPCSparseMatrix_local(rowptr, colidx, vals, len(rowptr) - 1 if ncols is None else ncols, B)


def _linear_solve(hp, B, solve, A, dense, bg, x0g, wg, combo, limit_of, **kw):
    """One solve with (b, x0, weights) on the combo's variants: the true residual within the convergence test's bound, and x, the
    history and the info bit-equal to the same solve on fresh tensors of the same values."""
    runs = []
    for variants in (combo, ("fresh",) * 3):
        pb, b = _vec_or_none(hp, B, bg, variants[0])
        p0, x0 = _vec_or_none(hp, B, x0g, variants[1])
        pw, w = _vec_or_none(hp, B, wg, variants[2])
        args = dict(kw)
        if x0 is not None:
            args["x0"] = x0
        if w is not None:
            args["M"] = w
        x, info = solve(A, b, **args)
        for p in (pb, p0, pw):
            if p is not None:
                p.unchanged()
        runs.append((x.local_values().copy(), info))
    (xv, info), (xf, info_f) = runs
    assert info.converged, info
    true, limit = limit_of(bg - dense @ xv)
    print(f"{solve.__name__} {combo}: {info.status} at {info.iterations}, true residual {true:.3e}, bound {limit:.3e}")
    assert true <= limit, (combo, true, limit)
    _same_bits(xv, xf, f"{solve.__name__} x {combo}")
    assert info == info_f, (combo, info, info_f)
    _same_info(info, info_f, f"{solve.__name__} {combo}")


SOLVER_COMBOS = vo.combos(*[vo.VECTOR_F64] * 3)
SIZE = pc.SIZES[0]                                               # 16 x 16: the smallest case of every linear solver's file


@pytest.fixture(scope="module")
def spd(orc):
    rowptr, colidx, vals, b = pc.scaled_poisson(orc, *SIZE)
    return dict(csr=(rowptr, colidx, vals), b=b, dense=bc.dense_of(rowptr, colidx, vals), dinv=1.0 / pc.host_diag(rowptr, colidx, vals))


@pytest.fixture(scope="module")
def nonsym(orc):
    rowptr, colidx, vals, b = bc.convection_diffusion(orc, *SIZE)
    return dict(csr=(rowptr, colidx, vals), b=b, dense=bc.dense_of(rowptr, colidx, vals), dinv=1.0 / pc.host_diag(rowptr, colidx, vals))


def _rel_to(bg):
    bn = float(np.linalg.norm(bg))
    return lambda r: (float(np.linalg.norm(r)) / bn, pc.TRUE_RES_RTOL)


@pytest.mark.parametrize("combo", SOLVER_COMBOS, ids=_ids)
def test_cg_with_view_operands(hp, backends, spd, combo):
    B = backends["i32"]
    A = _csr_matrix(hp, B, *spd["csr"])
    x0g = np.full(len(spd["b"]), 1e-3)
    _linear_solve(hp, B, hp.cg, A, spd["dense"], spd["b"], x0g, spd["dinv"], combo, _rel_to(spd["b"]), rtol=1e-8)
    if combo[2] == "fresh":                                      # plain CG: no weights
        _linear_solve(hp, B, hp.cg, A, spd["dense"], spd["b"], x0g, None, combo, _rel_to(spd["b"]), rtol=1e-8)
    hp.clear_plan_cache()


@pytest.mark.parametrize("combo", SOLVER_COMBOS, ids=_ids)
def test_bicgstab_with_view_operands(hp, backends, nonsym, combo):
    B = backends["i32"]
    A = _csr_matrix(hp, B, *nonsym["csr"])
    x0g = np.full(len(nonsym["b"]), 1e-3)
    _linear_solve(hp, B, hp.bicgstab, A, nonsym["dense"], nonsym["b"], x0g, nonsym["dinv"], combo, _rel_to(nonsym["b"]), rtol=1e-8)
    hp.clear_plan_cache()


@pytest.mark.parametrize("combo", SOLVER_COMBOS, ids=_ids)
def test_gmres_with_view_operands(hp, backends, nonsym, combo):
    B = backends["i32"]
    A = _csr_matrix(hp, B, *nonsym["csr"])
    x0g = np.full(len(nonsym["b"]), 1e-3)
    _linear_solve(hp, B, hp.gmres, A, nonsym["dense"], nonsym["b"], x0g, nonsym["dinv"], combo, _rel_to(nonsym["b"]), rtol=1e-8)
    if combo[1:] == ("fresh", "fresh"):                          # from x0 = 0: b goes straight to the first residual kernel
        _linear_solve(hp, B, hp.gmres, A, nonsym["dense"], nonsym["b"], None, None, combo, _rel_to(nonsym["b"]), rtol=1e-8)
    hp.clear_plan_cache()


@pytest.mark.parametrize("combo", SOLVER_COMBOS, ids=_ids)
def test_minres_with_view_operands(hp, orc, backends, combo):
    """The scaled saddle-point case with its Jacobi weights as a vector; the bound is the M-norm one of the convergence test."""
    B = backends["i32"]
    rowptr, colidx, vals, bg = mc.scaled_saddle(orc, *SIZE)
    dinv = mc.jacobi(rowptr, colidx, vals)
    A = _csr_matrix(hp, B, rowptr, colidx, vals)
    dense = mc.dense_of(rowptr, colidx, vals)
    limit = 1e-8 * mc.m_norm(bg, dinv)
    _linear_solve(hp, B, hp.minres, A, dense, bg, np.full(len(bg), 1e-3), dinv, combo,
                  lambda r: (mc.m_norm(r, dinv), pc.TRUE_RES_FACTOR * limit), rtol=1e-8)
    hp.clear_plan_cache()


@pytest.mark.parametrize("combo", vo.combos(*[vo.VECTOR_F64] * 2), ids=_ids)
def test_lsqr_with_view_operands(hp, orc, backends, combo):
    """The wide (consistent) case, b on the rows and x0 on the columns."""
    B = backends["i32"]
    rowptr, colidx, vals, ncols, bg = lc.wide(orc, *SIZE)
    A = _csr_matrix(hp, B, rowptr, colidx, vals, ncols)
    dense = lc.dense_of(rowptr, colidx, vals, ncols)
    runs = []
    for variants in (combo, ("fresh", "fresh")):
        pb, b = _vec_or_none(hp, B, bg, variants[0])
        p0, x0 = _vec_or_none(hp, B, np.full(ncols, 1e-3), variants[1])
        x, info = hp.lsqr(A, b, x0=x0)
        pb.unchanged(), p0.unchanged()
        runs.append((x.local_values().copy(), info))
    (xv, info), (xf, info_f) = runs
    assert info.converged and info.status == "converged"
    assert np.linalg.norm(bg - dense @ xv) <= pc.TRUE_RES_RTOL * np.linalg.norm(bg)
    _same_bits(xv, xf, f"lsqr x {combo}")
    assert info == info_f
    _same_info(info, info_f, f"lsqr {combo}")
    hp.clear_plan_cache()


@pytest.mark.parametrize("variant", vo.VECTOR_F64)
def test_eigsh_with_a_start_vector_view(hp, orc, backends, variant):
    B = backends["i32"]
    (name, size), k, ncv, _ = ec.CONVERGENCE[1]                  # plain Poisson 24 x 20, k = 1, ncv = 8: the smallest
    rowptr, colidx, vals = ec.plain_poisson(orc, *size)
    n = len(rowptr) - 1
    A = _csr_matrix(hp, B, rowptr, colidx, vals)
    dense = bc.dense_of(rowptr, colidx, vals)
    runs = []
    for v in (variant, "fresh"):
        p0, v0 = _vec_or_none(hp, B, ec.start_vector(n, 1), v)
        vals_, X, info = hp.eigsh(A, k=k, which="LA", ncv=ncv, tol=ec.TOL, v0=v0)
        p0.unchanged()
        runs.append((vals_, X.gather().copy(), info))
    (got, Xh, info), (got_f, Xf, info_f) = runs
    assert info.converged
    true = np.linalg.norm(dense @ Xh - Xh * got[None, :], axis=0)
    assert true.max() / (ec.TOL * info.anorm) <= pc.TRUE_RES_FACTOR
    _same_bits(got, got_f, "eigsh values"), _same_bits(Xh, Xf, "eigsh vectors")
    _same_info(info, info_f, "eigsh")                            # iterations, restarts, status, residual_norms, history, anorm
    assert len(info.history) == info.restarts + 1 and info.anorm > 0
    hp.clear_plan_cache()


@pytest.mark.parametrize("variant", vo.VECTOR_F64)
def test_svds_with_a_start_vector_view(hp, orc, backends, variant):
    B = backends["i32"]
    name, k, ncv = sc.CONVERGENCE[1]                             # tall, k = 1, ncv = 8
    M = sc.matrix(orc, name)
    A = _csr_matrix(hp, B, *M)
    sv = sc.dense_singular_values(*M)
    runs = []
    for v in (variant, "fresh"):
        p0, v0 = _vec_or_none(hp, B, sc.start_vector(M[3], 1), v)
        U, s, V, info = hp.svds(A, k=k, ncv=ncv, tol=sc.TOL, v0=v0)
        p0.unchanged()
        runs.append((U.local_values().copy(), s, V.local_values().copy(), info))
    (Uh, s, Vh, info), (Uf, s_f, Vf, info_f) = runs
    assert info.converged
    f = sc.figures(*M, Uh, s, Vh, info, sv)
    assert f["res"] <= pc.TRUE_RES_FACTOR and f["err"] <= sc.VAL_RTOL
    _same_bits(s, s_f, "svds values"), _same_bits(Uh, Uf, "svds U"), _same_bits(Vh, Vf, "svds V")
    _same_info(info, info_f, "svds")                             # iterations, restarts, status, residual_norms, history, anorm
    assert len(info.history) == info.restarts + 1 and info.anorm == s[0]
    hp.clear_plan_cache()


@pytest.mark.parametrize("combo", vo.combos(vo.MATRIX, vo.VECTOR_F64), ids=_ids)
def test_lobpcg_with_a_start_block_view_and_weight_view(hp, orc, backends, combo):
    """ddom257, k = 7, Jacobi weights handed in as a vector: positions (X0, M)."""
    B = backends["i32"]
    name, k, which, _ = next(c for c in lbc.CONVERGENCE if c[0] == "ddom257" and c[1] == 7)
    dense = lbc.ddom(257)
    ev = np.linalg.eigvalsh(dense)
    A = _csr_matrix(hp, B, *lbc.csr_of(dense)[:3])
    X0g, wg = lbc.start_block(257, k), lbc.jacobi_weights(dense)
    runs = []
    for cm, cw in (combo, ("fresh", "fresh")):
        px = Placed(np.ascontiguousarray(X0g), cm, matrix=True)
        pw, w = _vec_or_none(hp, B, wg, cw)
        got, X, info = hp.lobpcg(A, k=k, which=which, X0=_hmat(hp, B, px), M=w, tol=lbc.TOL)
        px.unchanged(), pw.unchanged()
        runs.append((got, X.gather().copy(), info))
    (got, Xh, info), (got_f, Xf, info_f) = runs
    err, res, orth, est = lbc.figures(dense, ev, got, Xh, dict(anorm=info.anorm, residual_norms=info.residual_norms), k, which)
    assert info.converged and res <= pc.TRUE_RES_FACTOR and err <= 2 * lbc.TOL and orth <= lbc.ORTH_TOL
    _same_bits(got, got_f, "lobpcg values"), _same_bits(Xh, Xf, "lobpcg vectors")
    _same_info(info, info_f, "lobpcg")                           # iterations, status, residual_norms, history, anorm
    assert len(info.history) == info.iterations and info.anorm > 0
    hp.clear_plan_cache()


# ---- 9. the preconditioner objects: apply and cg with M = hp.fsai(A) / hp.amg(A) -------------------------------------------------------
PRECONDITIONERS = ("fsai", "amg")


def _preconditioner(hp, kind, A):
    """hp.amg at coarse_size = 8: 256 -> 37 -> 4 rows on the 16 x 16 case, so the cycle runs both smoother kernels on two levels
    and the dense last level."""
    return hp.fsai(A) if kind == "fsai" else hp.amg(A, coarse_size=8)


@pytest.mark.parametrize("kind", PRECONDITIONERS)
@pytest.mark.parametrize("combo", vo.combos(vo.VECTOR_F64, vo.VECTOR_F64), ids=_ids)
def test_preconditioner_apply_on_views(hp, backends, spd, kind, combo):
    """``M.apply(r, out=out)``, positions (r, out): out holds the bits of the all-fresh call in the caller's buffer, r and the
    poison around both are untouched, and the call returns ``out`` itself."""
    B = backends["i32"]
    A = _csr_matrix(hp, B, *spd["csr"])
    M = _preconditioner(hp, kind, A)
    n = len(spd["b"])
    rg = _values(n, F64, 61)
    want = M.apply(_hvec(hp, B, Placed(rg, "fresh"))).local_values().copy()
    assert np.isfinite(want).all() and want.any()
    pr, po = Placed(rg, combo[0]), Placed(np.full(n, 7.0), combo[1])
    out = _hvec(hp, B, po)
    assert M.apply(_hvec(hp, B, pr), out=out) is out
    pr.unchanged()
    po.holds(want)
    hp.clear_plan_cache()


@pytest.mark.parametrize("kind", PRECONDITIONERS)
@pytest.mark.parametrize("combo", vo.combos(vo.VECTOR_F64, vo.VECTOR_F64), ids=_ids)
def test_cg_with_a_preconditioner_object_and_view_operands(hp, backends, spd, kind, combo):
    """hp.cg(A, b, x0=..., M=hp.fsai(A) or hp.amg(A)), positions (b, x0)."""
    B = backends["i32"]
    A = _csr_matrix(hp, B, *spd["csr"])
    M = _preconditioner(hp, kind, A)
    x0g = np.full(len(spd["b"]), 1e-3)
    _linear_solve(hp, B, hp.cg, A, spd["dense"], spd["b"], x0g, None, combo + ("fresh",), _rel_to(spd["b"]), rtol=1e-8, M=M)
    hp.clear_plan_cache()


def test_preconditioners_of_a_matrix_built_on_a_value_view(hp, backends, spd):
    """``HPCSparseMatrix_local_device`` keeps the caller's value tensor as it is: A on an ``nzval`` 8 bytes off a 16-byte boundary.
    Every level of hp.amg(A) and the G of hp.fsai(A) have the bits of the build on fresh storage; the values and the poison
    around them are untouched."""
    import torch
    B = backends["i32"]
    rowptr, colidx, vals = spd["csr"]
    n = len(rowptr) - 1
    built = {}
    for variant in ("off8", "fresh"):
        pv = Placed(np.asarray(vals, dtype=np.float64), variant)
        A = hp.HPCSparseMatrix_local_device(torch.from_numpy(np.array(rowptr, dtype=np.int64)).cuda(),
                                            torch.from_numpy(np.array(colidx, dtype=np.int64)).cuda(), pv.t, n, B)
        assert A.nzval.data_ptr() == pv.t.data_ptr() and A.nzval.data_ptr() % 16 == pv.promise[0], variant
        M, F = hp.amg(A, coarse_size=8), hp.fsai(A)
        pv.unchanged()
        built[variant] = (M, F)
    (M, F), (Mf, Ff) = built["off8"], built["fresh"]
    assert [l.n for l in M.levels] == [l.n for l in Mf.levels] and len(M.levels) >= 3
    host = lambda t: t.cpu().numpy()
    for k, (a, b) in enumerate(zip(M.levels, Mf.levels)):
        _same_bits(host(a.A.nzval), host(b.A.nzval), f"level {k} A")
        _same_bits(a.s.local_values(), b.s.local_values(), f"level {k} s")
        assert (a.w, a.rho, a.n_roots, a.rounds) == (b.w, b.rho, b.n_roots, b.rounds), k
        assert (a.P is None) == (b.P is None) and (a.inverse is None) == (b.inverse is None), k
        if a.P is not None:
            assert np.array_equal(host(a.aggregates), host(b.aggregates)), k
            _same_bits(host(a.P.nzval), host(b.P.nzval), f"level {k} P")
            _same_bits(host(a.Pt.nzval), host(b.Pt.nzval), f"level {k} Pt")
        if a.inverse is not None:
            _same_bits(a.inverse.local_values(), b.inverse.local_values(), f"level {k} inverse")
    assert np.array_equal(host(F.G.rowptr_target), host(Ff.G.rowptr_target)) and F.max_row == Ff.max_row
    _same_bits(host(F.G.nzval), host(Ff.G.nzval), "G")
    _same_bits(host(F.Gt.nzval), host(Ff.Gt.nzval), "Gt")
    hp.clear_plan_cache()
