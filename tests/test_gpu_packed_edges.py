"""The opt-in packed copy (csrc/packed.hip: 16-bit block-relative columns + 8-bit value codes) past its first pass, at the edges
of its window and of its dictionary, on the raw entry points, through the host layer, under ``HPCLA_SPMV_PACKED=1`` and across
ranks.  The matrices and ``packed_walk``, a numpy restatement of the kernel's pass loop, are in tests/_packed_cases.py;
tests/test_packed_cases.py shows on the CPU that every case has the property it is named after and that the walk gives the
oracle's bits on it, so a failure here is the kernel's.

Only two limits are used:
  * y: bit equality (``np.array_equal`` on the int64 view) with ``orc.spmv``, the stored-order loop of src/sparse.jl:2055-2066
    -- the packed kernel multiplies the same two doubles per entry and adds them in the same order, in however many passes;
  * scalars (``dot_partial`` per block, the fused ``mul_dot_``): ``RTOL_RED * |x|.|y|`` of the rows summed, the bound
    tests/test_gpu_parity.py uses for the fused scalar (1e-12, BASELINE.json).
Every test that expects the packed kernel asserts that it ran: ``hpcla_packed_create_i32`` returned 0 and left a handle, or
``enable_packed`` is True (``packed_reason`` shown otherwise).  y starts as NaN everywhere, x lies between NaN guards.

What a plausible slip in ``spmv_packed_kernel`` would break, by group (the same slip made in ``packed_walk`` fails
tests/test_packed_cases.py::test_a_slip_in_the_walk_is_seen):
  * pass edges -- ``double acc = 0.0;`` moved into the pass loop (no carry); ``g = pa + c + e0`` with p0 for pa; the clamps
    ``a = lo > c ? lo : c`` and ``e = hi < c + n ? hi : c + n``;
  * block lists -- ``blk = block_list ? block_list[blockIdx.x] : blockIdx.x`` and ``dot_partial[blk]``;
  * neighbour octets -- ``lo = rowptr[r0 + tid] - base - pa`` taken as 0 for the first lane, or the index clamp dropped;
  * dictionary -- ``s_dict[(cd >> (8 * k)) & 0xff]`` with a narrower mask or ``if (tid < ndict)`` off by one; on the host
    ``take = n_missing < CAP ? n_missing : CAP``;
  * window -- ``r0 + (int)dc[k]`` read unsigned; the encoder's range test off by one at -32768 / +32767.

Measured on the MI355X: the 30 tests without ranks take 6.2 s of wall time together (the child of the environment switch 2.1 s,
the first test 1.8 s with the library's start, each window case 0.4 s, everything else below 0.1 s); the rank tests 3.1 s
(2 ranks) and 2.8 s (3 ranks), about what test_qr_across_ranks takes."""
import ctypes
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _packed_cases as pc  # noqa: E402
from _packed_cases import RPB, eligible_np  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL_RED = 1e-12               # BASELINE.json: 1e-12 relative for fp64 reductions (tests/test_gpu_parity.py)
UNSUPPORTED = -5               # HPCLA_ERR_UNSUPPORTED (include/hpcla_rocm.h)
GUARD = 64
RANK_WORKER = os.path.join(ROOT, "tests", "_multirank_packed_worker.py")


@lru_cache(maxsize=None)
def case(name, *args):
    """One generated case per session, read-only."""
    out = getattr(pc, name)(*args)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def _reference(name, *args):
    """(x, y of the oracle) of a square case, computed once; x has one entry more than columns are owned (window 'ghost')."""
    from oracle import oracle as orc
    rowptr, col, vals = case(name, *args)[:3]
    n = len(rowptr) - 1
    x = orc.fill_uniform(0, n + 1, orc.SEED_X) - 0.5
    if name == "neighbour_octets":
        x[0] = x[n - 1] = np.nan                           # the two clamp targets
    y = orc.spmv(rowptr.astype(np.int32), col.astype(np.int32), vals, x)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class Raw:
    """A case on the device for the raw entry points with index_base `base`: x between NaN guards, every y NaN at first."""

    def __init__(self, hp, rowptr, col, vals, x, n_own, base):
        import torch
        self.hp, self.torch, self.lib = hp, torch, hp._capi.load()
        self.s = torch.cuda.current_stream().cuda_stream
        self.n, self.nnz, self.n_own, self.base = len(rowptr) - 1, len(col), n_own, base
        self.rp = torch.tensor((rowptr + base).astype(np.int32), device="cuda")
        self.cv = torch.tensor((col + base).astype(np.int32), device="cuda")
        self.nz = torch.tensor(np.asarray(vals), device="cuda")
        self.xbuf = torch.full((n_own + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        self.xbuf[GUARD:GUARD + n_own] = torch.tensor(np.asarray(x[:n_own]), device="cuda")
        self.x = self.xbuf[GUARD:GUARD + n_own]
        self.handles = []

    def _list(self, blocks):
        if blocks is None:
            return None, None, 0
        t = self.torch.tensor(list(blocks), dtype=self.torch.int32, device="cuda")
        return t, t.data_ptr(), len(blocks)

    def create(self, blocks=None):
        """(status, handle, reason)"""
        h = ctypes.c_void_p()
        keep, ptr, nb = self._list(blocks)
        rc = self.lib.hpcla_packed_create_i32(ctypes.byref(h), self.rp.data_ptr(), self.cv.data_ptr(), self.nz.data_ptr(),
                                              self.n, self.nnz, self.n_own, self.base, ptr, nb, self.s)
        self.torch.cuda.synchronize()
        reason = self.hp._capi.last_error() if rc else ""
        if rc == 0:
            assert h.value, "create returned OK and no handle"
            self.handles.append(h)
        return rc, h, reason

    def must_create(self, blocks=None):
        rc, h, reason = self.create(blocks)
        assert rc == 0, f"hpcla_packed_create_i32 refused ({rc}): {reason}"
        return h

    def ndict(self, h):
        nbytes, nd = ctypes.c_int64(), ctypes.c_int()
        self.hp._capi.call("hpcla_packed_info", h, ctypes.byref(nbytes), ctypes.byref(nd))
        assert 3 * self.nnz <= nbytes.value <= 3 * (self.nnz + 16) + 256 * 8
        return nd.value

    def multiply(self, h, blocks=None, partial=None):
        y = self.torch.full((self.n,), float("nan"), dtype=self.torch.float64, device="cuda")
        keep, ptr, nb = self._list(blocks)
        self.hp._capi.call("hpcla_spmv_packed_f64_i32", h, self.rp.data_ptr(), self.x.data_ptr(), y.data_ptr(), self.base, ptr, nb,
                           None if partial is None else partial.data_ptr(), self.s)
        self.torch.cuda.synchronize()
        return y.cpu().numpy()

    def close(self):
        for h in self.handles:
            self.hp._capi.call("hpcla_packed_destroy", h)
        self.handles = []


def _raw(hp, name, *args, base=0):
    rowptr, col, vals = case(name, *args)[:3]
    x, want = _reference(name, *args)
    n_own = len(rowptr) - 1
    return Raw(hp, rowptr, col, vals, x, n_own, base), want


def _check_rows(got, want, blocks, what):
    """listed rows have the oracle's bits, every other row still holds the NaN it started with"""
    n = len(want)
    on = np.ones(n, dtype=bool) if blocks is None else np.isin(np.arange(n) // RPB, list(blocks))
    diff = np.flatnonzero(_bits(got[on]) != _bits(want[on]))
    assert len(diff) == 0, f"{what}: {len(diff)} listed rows differ from the oracle, first at listed row {diff[:5]}"
    assert np.all(np.isnan(got[~on])), f"{what}: {int((~np.isnan(got[~on])).sum())} rows outside the list were written"


def _good_create_and_product(hp, what):
    """after a refusal: the next create and product are as if nothing had happened"""
    r, want = _raw(hp, "stencil9", 40, 40)
    try:
        _check_rows(r.multiply(r.must_create()), want, None, f"stencil9 after {what}")
    finally:
        r.close()


STENCILS = [("stencil9", 40, 40), ("stencil27", 12, 12, 12)]
MULTI_PASS = [("pass_edges",)] + STENCILS


# ---- raw entry points -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("name_args", MULTI_PASS, ids=lambda c: c[0])
def test_raw_rows_carried_across_passes(hp, name_args, base):
    """Blocks of 2047 ... 4097 entries from the octet-aligned start at p0 % 8 = 0, 3, 7, rows on, at and across pass
    boundaries, rows of 5000 entries in the first and the last lane, an empty block, a ragged last block; 9- and 27-point
    stencils (two and four passes per block).  Both index bases; a second call gives the same bits."""
    r, want = _raw(hp, *name_args, base=base)
    try:
        rowptr, _, vals = case(*name_args)[:3]
        assert max(pc.n_passes(rowptr, b) for b in range(pc.n_blocks(r.n))) >= 2
        h = r.must_create()
        assert r.ndict(h) == len(pc.bit_patterns(vals))
        first = r.multiply(h)
        _check_rows(first, want, None, f"{name_args[0]} base {base}")
        assert np.array_equal(_bits(r.multiply(h)), _bits(first)), "a second call gives other bits"
    finally:
        r.close()


@pytest.mark.parametrize("which", ["skip_third", "descending", "shuffled"])
def test_raw_block_lists(hp, which):
    """Create and multiply with a block list (every third block left out; the same list descending; all blocks shuffled):
    listed rows exact, the others untouched.  Also a whole copy multiplied under the list."""
    r, want = _raw(hp, "pass_edges")
    try:
        nb = pc.n_blocks(r.n)
        blocks = {"skip_third": pc.skip_every_third(nb), "descending": pc.skip_every_third(nb)[::-1], "shuffled": pc.shuffled(nb)}[which]
        _check_rows(r.multiply(r.must_create(blocks), blocks), want, blocks, f"{which}: listed copy")
        _check_rows(r.multiply(r.must_create(), blocks), want, blocks, f"{which}: whole copy")
    finally:
        r.close()


def test_raw_octets_shared_with_the_neighbouring_blocks(hp):
    """Every block's first and last octet also holds entries of its neighbours, whose deltas point below 0 and past n_own
    from here: the clamp sends them to x[0] and x[n_own - 1], which hold NaN (no row stores either column), and behind the
    clamp targets lie the NaN guards of x.  The products are formed and must not be summed: y is finite and exact."""
    r, want = _raw(hp, "neighbour_octets")
    try:
        listed = case("neighbour_octets")[3]
        assert np.all(np.isfinite(want)) and bool(r.torch.isnan(r.x[0])) and bool(r.torch.isnan(r.x[-1]))
        h = r.must_create()
        _check_rows(r.multiply(h), want, None, "whole matrix")
        _check_rows(r.multiply(h, listed), want, listed, "blocks 1, 3, 5")
    finally:
        r.close()


@pytest.mark.parametrize("order", ["all", "shuffled"])
def test_raw_dot_partial_of_every_block(hp, order):
    """The epilogue's per-block x.y (index = the block, not its place in the list), the ragged last block of 100 rows with
    two empty waves included; same bits on a second call."""
    r, want = _raw(hp, "pass_edges")
    try:
        x = _reference("pass_edges")[0][:r.n]
        nb = pc.n_blocks(r.n)
        blocks = None if order == "all" else pc.shuffled(nb)
        h = r.must_create()
        got = []
        for _ in range(2):
            partial = r.torch.full((nb,), float("nan"), dtype=r.torch.float64, device="cuda")
            _check_rows(r.multiply(h, blocks, partial), want, blocks, "y next to dot_partial")
            got.append(partial.cpu().numpy())
        assert np.array_equal(_bits(got[0]), _bits(got[1])), "dot_partial differs between two calls"
        for b in range(nb):
            rows = slice(RPB * b, min(RPB * b + RPB, r.n))
            ref = float(np.sum(want[rows].astype(np.longdouble) * x[rows].astype(np.longdouble)))
            scale = float(np.abs(want[rows]) @ np.abs(x[rows]))
            print(f"block {b}: partial {got[0][b]!r} reference {ref!r} bound {RTOL_RED * scale:.3e}")
            assert abs(got[0][b] - ref) <= RTOL_RED * scale, (b, got[0][b], ref)
    finally:
        r.close()


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("which", ["edges", "past_low", "past_high", "ghost"])
def test_raw_window_edges(hp, which, base):
    """Deltas of exactly -32768 and +32767 (in one block, in one row) are packed and decoded exactly.  One beyond either, or
    a column that is not owned, in a listed block: refused with the window reason and no handle; with that block left out of
    the list the copy is made and the listed rows are exact."""
    rowptr, col, vals, n_own, bad = case("window_edges", which)
    x, want = _reference("window_edges", which)
    assert eligible_np(rowptr, col, n_own) == (which == "edges")
    r = Raw(hp, rowptr, col, vals, x, n_own, base)
    try:
        if which == "edges":
            h = r.must_create()
            assert r.ndict(h) == 5
            _check_rows(r.multiply(h), want, None, "edges")
            return
        rc, h, reason = r.create()
        assert rc == UNSUPPORTED and "window" in reason and not h.value, (rc, reason, h.value)
        others = [b for b in range(pc.n_blocks(r.n)) if b != bad]
        assert eligible_np(rowptr, col, n_own, blocks=others)
        _check_rows(r.multiply(r.must_create(others), others), want, others, f"{which} without block {bad}")
    finally:
        r.close()
    _good_create_and_product(hp, f"the refusal of {which}")


@pytest.mark.parametrize("kind", ["one", "full", "flood", "rounds", "over"])
def test_raw_dictionary(hp, kind):
    """One value; 256 values with code 255 in second passes; a seed sample of one value and 60 416 misses of three others
    (the bounded miss list overflows); 200 late values in runs (several rounds of extension): each packed with exactly its
    number of values and multiplied exactly.  257 values, the last one only behind the sample and 5000 times: refused."""
    rowptr, col, vals, nd = case("dictionary", kind)
    r, want = _raw(hp, "dictionary", kind)
    try:
        if nd is None:
            rc, h, reason = r.create()
            assert rc == UNSUPPORTED and "distinct" in reason and not h.value, (rc, reason, h.value)
        else:
            h = r.must_create()
            assert r.ndict(h) == nd == len(pc.bit_patterns(vals))
            _check_rows(r.multiply(h), want, None, kind)
    finally:
        r.close()
    if nd is None:
        _good_create_and_product(hp, "the refusal of 257 values")


# ---- host layer -------------------------------------------------------------------------------------------------------------
def _host_products(hp, A, x, with_dot):
    """(bits of A @ x, of mul_(y, A, x) into a NaN-filled y, of mul_dot_'s y, mul_dot_'s scalar)"""
    import torch
    out = [(A @ x).local_values().copy()]
    y = hp.HPCVector.zeros(A.row_partition, A.backend)
    y.v.fill_(float("nan"))
    hp.mul_(y, A, x)
    out.append(y.local_values().copy())
    if with_dot:
        y.v.fill_(float("nan"))
        s = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        hp.mul_dot_(y, A, x, s)
        torch.cuda.synchronize()
        out += [y.local_values().copy(), float(s.item())]
    return out


@pytest.mark.parametrize("name_args", MULTI_PASS, ids=lambda c: c[0])
def test_host_layer_products_with_and_without_the_packed_copy(hp, orc, gpu_backend_i32, name_args):
    """A.enable_packed(x), then A @ x, mul_ and mul_dot_: the oracle's bits, and those of the same calls after
    disable_packed(); the fused scalar within RTOL_RED * |x|.|y| on both paths."""
    rowptr, col, vals = case(*name_args)[:3]
    n = len(rowptr) - 1
    xg, want = _reference(*name_args)
    xg = np.array(xg[:n])
    A = hp.HPCSparseMatrix_local(rowptr, col, np.array(vals), n, gpu_backend_i32)
    x = hp.HPCVector.from_global(xg, gpu_backend_i32)
    plan = hp.get_vector_plan(A, x)
    assert A.enable_packed(x) is True, A.packed_reason
    assert A._packed.get(plan.key) is not None and A._packed_for(plan) is not None
    packed = _host_products(hp, A, x, True)
    A.disable_packed()
    assert A._packed_for(plan) is None
    plain = _host_products(hp, A, x, True)
    ref = orc.dot([xg], [np.array(want)])
    bound = RTOL_RED * float(np.abs(xg) @ np.abs(want))
    for leg, res in (("packed", packed), ("CSR", plain)):
        for what, y in zip(("A @ x", "mul_", "mul_dot_"), res[:3]):
            diff = np.flatnonzero(_bits(y) != _bits(want))
            assert len(diff) == 0, f"{name_args[0]} {leg} {what}: {len(diff)} rows differ, first {diff[:5]}"
        print(f"{name_args[0]} {leg}: x.Ax {res[3]!r} reference {ref!r} bound {bound:.3e}")
        assert abs(res[3] - ref) <= bound, (leg, res[3], ref)
    hp.clear_plan_cache()


def test_host_layer_rectangular(hp, orc, gpu_backend_i32):
    """1000 x 1300, two passes per block, the last rows reading columns behind the square part."""
    rowptr, col, vals, ncols = case("rectangular")
    xg = orc.fill_uniform(0, ncols, orc.SEED_X) - 0.5
    want = orc.spmv(rowptr.astype(np.int32), col.astype(np.int32), vals, xg)
    A = hp.HPCSparseMatrix_local(rowptr, col, np.array(vals), ncols, gpu_backend_i32)
    x = hp.HPCVector.from_global(xg, gpu_backend_i32)
    assert A.shape == (len(rowptr) - 1, ncols)
    plan = hp.get_vector_plan(A, x)
    ok = A.enable_packed(x)
    print(f"rectangular: enable_packed {ok} {A.packed_reason!r}")
    assert (A._packed_for(plan) is not None) == ok
    for y in _host_products(hp, A, x, False):
        assert np.array_equal(_bits(y), _bits(want)), f"rectangular, packed copy {ok}"
    assert ok is True, f"a matrix inside the window with 4 values is packable: {A.packed_reason}"
    A.disable_packed()
    for y in _host_products(hp, A, x, False):
        assert np.array_equal(_bits(y), _bits(want)), "rectangular, CSR"
    hp.clear_plan_cache()


# ---- HPCLA_SPMV_PACKED=1 -----------------------------------------------------------------------------------------------------
_ENV_CHILD = """
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import hpcla_amd as hp
import _packed_cases as pc
from oracle import oracle as orc
assert os.environ["HPCLA_SPMV_PACKED"] == "1"
b = hp.backend_rocm_serial(np.float64, np.int32)
rowptr, col, vals = pc.stencil9(40, 40)
n = len(rowptr) - 1
xg = (orc.fill_uniform(0, n + 1, orc.SEED_X) - 0.5)[:n]
A = hp.HPCSparseMatrix_local(rowptr, col, vals, n, b)
x = hp.HPCVector.from_global(xg, b)
assert not A._packed
y = (A @ x).local_values()
plan = hp.get_vector_plan(A, x)
assert A._packed.get(plan.key) is not None, "no packed handle: " + repr(A.packed_reason)
print("fingerprint", pc.fingerprint(y))
"""


def test_environment_switch_packs_without_being_asked():
    """HPCLA_SPMV_PACKED=1 is read once when the package is imported: a fresh child multiplies the 9-point stencil without
    calling enable_packed, finds a packed handle on the matrix and prints a digest of y; the parent compares it with the
    oracle's."""
    _, want = _reference("stencil9", 40, 40)
    env = dict(os.environ, HPCLA_SPMV_PACKED="1")
    out = subprocess.run([sys.executable, "-c", _ENV_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("fingerprint ")]
    assert lines == [["fingerprint", pc.fingerprint(want)]], out.stdout[-3000:]


# ---- ranks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_packed_interior_across_ranks(nranks):
    """Ranks sharing the GPU (the pattern of tests/test_gpu_qr.py::test_qr_across_ranks): multi-pass packed interior blocks,
    CSR boundary blocks, A @ x and mul_dot_ against the one-rank oracle; checks in tests/_multirank_packed_worker.py."""
    from hpcla_amd.launch import spawn_ranks
    env = {"HPCLA_PUSH_TIMEOUT_S": "30"}
    os.environ.pop("HPCLA_HALO_MODE", None)
    assert spawn_ranks([RANK_WORKER], nranks, env_extra=env, timeout=120, forward_rank0_stdout=False) == 0
