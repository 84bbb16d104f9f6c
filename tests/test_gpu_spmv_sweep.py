"""Sweep direction of repeated SpMV launches (csrc/spmv.hip: reversed_index, next_sweep).  A plain launch over a contiguous
run that repeats the calling thread's last one walks the row blocks downwards; every such order must be a bijection on the
run -- y prefilled with NaN and compared with ``np.array_equal`` against the oracle's stored-order sum after EVERY launch --
and ``hpcla_spmv_last_sweep`` must show that both directions ran.  Shapes: a 50-wide 5-point grid cut to 1, 2, 7, 8, 9 and
133 row blocks whose last block holds 77 rows (133 = two spans of groups of 8 and a ragged tail of five blocks)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, "tests", "_sweep_direction_worker.py")
BLOCKS = (1, 2, 7, 8, 9, 133)
FORWARD, ALTERNATE, FROM_ENV = 0, 1, -1
_cases = {}


def case(orc, nblocks):
    """(rows, x, want) of the 50-wide grid's first 256 (nblocks - 1) + 77 rows; computed once per size and never written."""
    if nblocks not in _cases:
        n = 256 * (nblocks - 1) + 77
        ny = n // 50 + 1
        rows = orc.poisson2d_rows(50, ny, 0, n)
        x = orc.fill_uniform(0, 50 * ny, orc.SEED_X) - 0.5
        want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, x)
        for a in (rows.rowptr, rows.colidx, rows.vals, x, want):
            a.setflags(write=False)
        _cases[nblocks] = (rows, x, want)
    return _cases[nblocks]


def last_sweep(hp):
    rev = ctypes.c_int(-1)
    hp._capi.call("hpcla_spmv_last_sweep", ctypes.byref(rev))
    return int(rev.value)


@pytest.fixture
def sweep_mode(hp):
    """Sets the process-wide mode for a test (FROM_ENV: what HPCLA_SPMV_SWEEP says, as at load time) and puts that back."""
    def set_mode(mode):
        if mode == FROM_ENV:
            hp._capi.apply_spmv_sweep_env()
        else:
            hp._capi.call("hpcla_set_spmv_sweep", mode)
    yield set_mode
    hp._capi.apply_spmv_sweep_env()


class Device:
    """The case's arrays on the device, for one entry point; launch(y) makes one product into y."""

    def __init__(self, hp, orc, nblocks, entry, vals=None):
        import torch
        self.hp, self.entry = hp, entry
        rows, x, want = case(orc, nblocks)
        self.n, self.nnz, self.want = len(rows.rowptr) - 1, len(rows.colidx), want
        Ti = np.int64 if entry.endswith("_i64") else np.int32
        self.rp = torch.from_numpy(rows.rowptr.astype(Ti)).cuda()
        self.cv = torch.from_numpy(rows.colidx.astype(Ti)).cuda()
        self.nz = torch.from_numpy(np.array(rows.vals if vals is None else vals)).cuda()
        self.x = torch.from_numpy(np.array(x)).cuda()
        self.s = torch.cuda.current_stream().cuda_stream
        self.c16 = self.h = None
        lib = hp._capi.load()
        if "cols16" in entry or "patterns" in entry:
            self.c16 = torch.empty(lib.hpcla_cols16_padded_len(self.nnz), dtype=torch.int16, device="cuda")
            bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
            hp._capi.call("hpcla_cols16_encode_i32", self.rp.data_ptr(), self.cv.data_ptr(), self.n, self.nnz, int(self.x.numel()),
                          0, None, 0, self.c16.data_ptr(), bad.data_ptr(), self.s)
            assert int(bad.item()) == 0
        if "patterns" in entry:
            self.h = ctypes.c_void_p()
            hp._capi.call("hpcla_block_patterns_create_i32", ctypes.byref(self.h), self.rp.data_ptr(), self.c16.data_ptr(), self.n,
                          self.nnz, 0, None, -1, 0, 0, self.s)
            assert self.h, "the 5-point grid repeats its patterns: the library must build a table"

    def fresh(self):
        import torch
        return torch.full((self.n,), float("nan"), dtype=torch.float64, device="cuda")

    def launch(self, y, block_list=None):
        p = lambda t: t.data_ptr()        # noqa: E731
        bl = (p(block_list), int(block_list.numel())) if block_list is not None else (None, 0)
        if self.h is not None:
            self.hp._capi.call(self.entry, p(self.rp), p(self.c16), self.h, p(self.nz), p(self.x), p(y), self.n, self.nnz, 0, *bl, self.s)
        elif self.c16 is not None:
            self.hp._capi.call(self.entry, p(self.rp), p(self.c16), p(self.nz), p(self.x), p(y), self.n, self.nnz, 0, *bl, self.s)
        else:
            assert block_list is None
            self.hp._capi.call(self.entry, p(self.rp), p(self.cv), p(self.nz), p(self.x), p(y), self.n, self.nnz, 0, self.s)

    def close(self):
        if self.h is not None:
            self.hp._capi.call("hpcla_block_patterns_destroy", self.h)
            self.h = None
        self.hp._capi.load().hpcla_spmv_block_order_hint(ctypes.c_void_p(self.rp.data_ptr()), 0)


ENTRIES = ("hpcla_spmv_csr_f64_i32", "hpcla_spmv_csr_f64_i64", "hpcla_spmv_cols16_f64_i32", "hpcla_spmv_patterns_f64_i32")


@pytest.mark.parametrize("hint", [0, 8])
@pytest.mark.parametrize("nblocks", BLOCKS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_both_directions_are_bijections_with_the_oracles_bits(hp, orc, sweep_mode, entry, nblocks, hint):
    d = Device(hp, orc, nblocks, entry)
    try:
        hp._capi.call("hpcla_spmv_block_order_hint", d.rp.data_ptr(), hint)
        for mode, expect in ((ALTERNATE, [0, 1, 0, 1]), (FORWARD, [0, 0, 0, 0])):
            sweep_mode(mode)
            other = Device(hp, orc, 1, "hpcla_spmv_csr_f64_i32")      # another matrix in between: the next launch starts forwards
            other.launch(other.fresh())
            seen = []
            for k in range(4):
                y = d.fresh()
                d.launch(y)
                seen.append(last_sweep(hp))
                got = y.cpu().numpy()
                assert np.array_equal(got, d.want), f"launch {k} (reversed={seen[-1]}): {int((got != d.want).sum())} rows differ"
            assert seen == expect, (mode, seen)
    finally:
        d.close()


def test_run_launches_in_both_directions(hp, orc, sweep_mode):
    """The interior-run form (block_base >= 0).  The only public entries that launch a run without a halo plan are the plan-time
    tuners, which need 4096 row blocks before they measure: 4200 blocks, the run is blocks 7 ... 139 (133 of them).  Every
    launch of the tuner writes the complete product of the run into the scratch vector; under `forward` the last one went
    upwards, under `alternate` (an even number of launches from a forward start) downwards.  Rows outside the run keep NaN."""
    import torch
    nb, base, run = 4200, 7, 133
    n = 256 * (nb - 1) + 77
    ny = n // 50 + 1
    rows = orc.poisson2d_rows(50, ny, 0, n)
    x = orc.fill_uniform(0, 50 * ny, orc.SEED_X) - 0.5
    want = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), rows.vals, x)
    lib = hp._capi.load()
    s = torch.cuda.current_stream().cuda_stream
    rp = torch.from_numpy(rows.rowptr.astype(np.int32)).cuda()
    cv = torch.from_numpy(rows.colidx.astype(np.int32)).cuda()
    nz, xd = torch.from_numpy(rows.vals).cuda(), torch.from_numpy(x).cuda()
    c16 = torch.empty(lib.hpcla_cols16_padded_len(rows.nnz), dtype=torch.int16, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    hp._capi.call("hpcla_cols16_encode_i32", rp.data_ptr(), cv.data_ptr(), n, rows.nnz, 50 * ny, 0, None, 0, c16.data_ptr(),
                  bad.data_ptr(), s)
    assert int(bad.item()) == 0
    inside = (np.arange(n) // 256 >= base) & (np.arange(n) // 256 < base + run)
    try:
        for mode, expect in ((FORWARD, 0), (ALTERNATE, 1)):
            sweep_mode(mode)
            other = Device(hp, orc, 1, "hpcla_spmv_csr_f64_i32")      # another matrix in between: the tuner starts forwards
            other.launch(other.fresh())
            y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            chosen = ctypes.c_int(-1)
            hp._capi.call("hpcla_spmv_tune_block_order_cols16_f64_i32", rp.data_ptr(), c16.data_ptr(), nz.data_ptr(), xd.data_ptr(),
                          y.data_ptr(), n, rows.nnz, 0, base, run, s, ctypes.byref(chosen))
            assert chosen.value in (1, 8, 32, 64)
            assert last_sweep(hp) == expect
            got = y.cpu().numpy()
            assert np.array_equal(got[inside], want[inside]) and np.isnan(got[~inside]).all()
    finally:
        lib.hpcla_spmv_block_order_hint(ctypes.c_void_p(rp.data_ptr()), 0)


@pytest.mark.parametrize("entry", ["hpcla_spmv_cols16_f64_i32", "hpcla_spmv_patterns_f64_i32"])
def test_listed_launches_go_forwards_and_leave_the_record_alone(hp, orc, sweep_mode, entry):
    """hpcla_spmv_last_sweep reports the thread's last PLAIN launch: a listed launch in between changes neither what it reads
    nor the direction of the next plain launch, and writes the listed blocks only."""
    import torch
    sweep_mode(ALTERNATE)
    d = Device(hp, orc, 9, entry)
    try:
        some = torch.arange(0, 9, 2, dtype=torch.int32, device="cuda")
        listed = (np.arange(d.n) // 256) % 2 == 0
        seen = []
        for k in range(4):
            y = d.fresh()
            d.launch(y)
            seen.append(last_sweep(hp))
            assert np.array_equal(y.cpu().numpy(), d.want)
            ys = torch.full((d.n,), -7.0, dtype=torch.float64, device="cuda")
            d.launch(ys, block_list=some)
            assert last_sweep(hp) == seen[-1], "a listed launch moved the record"
            assert np.array_equal(ys.cpu().numpy(), np.where(listed, d.want, -7.0))
        assert seen == [0, 1, 0, 1]
    finally:
        d.close()


@pytest.mark.parametrize("nblocks", [9, 133])
def test_dot_epilogue_keeps_y_and_the_scalars_bits(hp, orc, sweep_mode, nblocks):
    import torch
    sweep_mode(ALTERNATE)
    d = Device(hp, orc, nblocks, "hpcla_spmv_csr_f64_i32")
    try:
        lib = hp._capi.load()
        hp._capi.call("hpcla_spmv_block_order_hint", d.rp.data_ptr(), 8)
        work = torch.empty(lib.hpcla_spmv_dot_work_bytes(d.n) // 8 + 1, dtype=torch.float64, device="cuda")
        seen, dots = [], []
        for _ in range(4):
            y, out = d.fresh(), torch.zeros(1, dtype=torch.float64, device="cuda")
            hp._capi.call("hpcla_spmv_dist_dot_f64_i32", None, None, d.rp.data_ptr(), d.cv.data_ptr(), d.nz.data_ptr(), d.x.data_ptr(),
                          d.n, y.data_ptr(), d.n, d.nnz, 0, None, 0, None, 0, out.data_ptr(), work.data_ptr(), d.s)
            seen.append(last_sweep(hp))
            assert np.array_equal(y.cpu().numpy(), d.want)
            dots.append(out.cpu().numpy().copy().view(np.int64)[0])
        assert seen == [0, 1, 0, 1]
        assert len(set(dots)) == 1, "x.y differs in bits between the directions: the partials must stay indexed by row block"
    finally:
        d.close()


def test_two_matrices_in_turn_and_two_value_arrays_stay_forwards(hp, orc, sweep_mode):
    sweep_mode(ALTERNATE)
    rows, _, _ = case(orc, 9)
    a = Device(hp, orc, 9, "hpcla_spmv_csr_f64_i32")
    b = Device(hp, orc, 9, "hpcla_spmv_csr_f64_i32")                  # equal shape, its own arrays
    v2 = rows.vals * 1.5
    want2 = orc.spmv(rows.rowptr.astype(np.int32), rows.colidx.astype(np.int32), v2, np.array(case(orc, 9)[1]))
    import torch
    nz2 = torch.from_numpy(v2).cuda()
    for k in range(3):
        for d in (a, b):
            y = d.fresh()
            d.launch(y)
            assert last_sweep(hp) == 0, "two matrices launched alternately keep the forward order"
            assert np.array_equal(y.cpu().numpy(), d.want)
    nz1 = a.nz
    for k in range(4):                                                # the same rowptr, another nzval
        a.nz, want = (nz2, want2) if k % 2 == 0 else (nz1, a.want)
        y = a.fresh()
        a.launch(y)
        assert last_sweep(hp) == 0, "same rowptr, different nzval: another matrix"
        assert np.array_equal(y.cpu().numpy(), want)
    a.nz = nz1


def test_switch_rejects_a_bad_mode(hp, sweep_mode):
    lib = hp._capi.load()
    assert lib.hpcla_set_spmv_sweep(2) != 0 and lib.hpcla_set_spmv_sweep(-2) != 0
    assert lib.hpcla_spmv_last_sweep(None) != 0


def test_host_layer_products_equal_a_forward_process(hp, orc, gpu_backend_i32, sweep_mode, tmp_path):
    """hp.mul_ four times on the 64 x 64 5-point matrix, with a pattern-table plan and under HPCLA_BLOCK_PATTERNS=0: every y
    has the bits of the first, both directions ran, and a fresh process under HPCLA_SPMV_SWEEP=forward -- which must report
    forwards throughout -- computes the same bits."""
    from _sweep_direction_worker import products
    sweep_mode(FROM_ENV)
    assert os.environ.get("HPCLA_SPMV_SWEEP", "alternate") != "forward"
    here = {}
    for patterns in (True, False):
        ys, dirs, plan = products(hp, orc, gpu_backend_i32, patterns)
        assert (plan.patterns is not None) == patterns and plan.cols16 is not None
        assert dirs in ([0, 1, 0, 1], [1, 0, 1, 0]), dirs           # (get_vector_plan may already have multiplied once)
        for y in ys[1:]:
            assert np.array_equal(y.view(np.int64), ys[0].view(np.int64))
        here[patterns] = ys[0]
    hp.clear_plan_cache()
    out = str(tmp_path / "forward.npz")
    env = dict(os.environ, HPCLA_SPMV_SWEEP="forward")
    env.pop("HPCLA_BLOCK_PATTERNS", None)
    subprocess.run([sys.executable, WORKER, out], check=True, env=env, timeout=300)
    with np.load(out, allow_pickle=False) as z:
        assert z["dirs_pat"].tolist() == [0, 0, 0, 0] and z["dirs_nopat"].tolist() == [0, 0, 0, 0]
        for k in range(4):
            assert np.array_equal(z["y_pat"][k].view(np.int64), here[True].view(np.int64))
            assert np.array_equal(z["y_nopat"][k].view(np.int64), here[False].view(np.int64))
