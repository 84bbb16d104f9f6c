"""transpose(X) * A and X * A for a sparse A, the parts that need no GPU: the host plans of the reverse halo and of
copy(transpose(X)) executed in numpy across 2, 3 and 8 gloo processes (tests/_dense_sparse_host_worker.py), and the C
ABI of csrc/spmm_t.hip as the header, the ctypes table and the built library describe it."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hpcla_amd  # noqa: E402,F401  (makes hpcla_amd.launch importable)

from tests.test_julia_binding_signatures import header_prototypes  # noqa: E402

SPMM_T = {"hpcla_spmm_t_struct_work_bytes": ("i64", ["i64", "i64", "i32"]),
          "hpcla_spmm_t_struct_i32": ("i32", ["ptr", "ptr", "i64", "i64", "i64", "ptr", "ptr", "ptr", "ptr", "i64", "ptr"]),
          "hpcla_spmm_t_struct_i64": ("i32", ["ptr", "ptr", "i64", "i64", "i64", "ptr", "ptr", "ptr", "ptr", "i64", "ptr"]),
          "hpcla_spmm_t_f64_i32": ("i32", ["ptr", "ptr", "ptr", "ptr", "i64", "ptr", "i64", "i32", "i64", "ptr", "i64", "i32", "ptr"]),
          "hpcla_spmm_t_f64_i64": ("i32", ["ptr", "ptr", "ptr", "ptr", "i64", "ptr", "i64", "i32", "i64", "ptr", "i64", "i32", "ptr"]),
          "hpcla_spmm_t_accumulate_f64": ("i32", ["ptr", "i64", "ptr", "i64", "ptr", "ptr", "ptr", "i64", "i64", "ptr"])}


@pytest.mark.parametrize("nranks", [2, 3, 8])
def test_host_plans_across_processes_gloo(nranks):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    from hpcla_amd.launch import free_port
    port = free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nranks}",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "_dense_sparse_host_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count(": OK") == nranks


def test_reverse_lists_on_one_rank_are_empty(hp):
    """One rank: every column is owned, nothing travels back, the split space is the global column space."""
    comm = hp.CommSerial()
    ci = np.array([0, 2, 3, 7], dtype=np.int64)
    h = hp.HostSpmmTPlan(ci, hp.uniform_partition(9, 1), comm)
    assert (h.n_own, h.n_ghost, h.ncols_split) == (9, 0, 9)
    np.testing.assert_array_equal(h.cmap, ci)
    assert h.back_ranks == [] and h.from_ranks == [] and h.n_recv == 0 and len(h.acc_rows) == 0
    L = hp.DenseTransposeLists(np.array([0, 5]), np.array([0, 3]), 0)
    assert (L.n_buf, L.local_src, L.local_dst, L.local_count) == (15, 0, 0, 15)
    assert L.blocks == [(0, 0, 5, 0)]


def test_header_declares_the_entries_and_ctypes_binds_them(hp):
    protos = header_prototypes()
    cls = {ctypes.c_void_p: "ptr", ctypes.c_int: "i32", ctypes.c_int64: "i64"}
    for name, (ret, params) in SPMM_T.items():
        assert protos.get(name) == (ret, params), (name, protos.get(name))
        assert [cls[t] for t in hp._capi._SIGNATURES[name]] == params
    assert hp._capi._RESTYPES["hpcla_spmm_t_struct_work_bytes"] is ctypes.c_int64
    out = subprocess.run(["nm", "-D", "--defined-only", hp._capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in SPMM_T:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


def test_argument_errors_and_work_size_without_a_gpu(hp):
    lib = hp._capi.load()
    assert lib.hpcla_spmm_t_struct_work_bytes(-1, 5, 0) == -1
    assert lib.hpcla_spmm_t_struct_work_bytes(1000, 500, 0) >= 2 * 4 * 1000
    assert lib.hpcla_spmm_t_struct_work_bytes(1000, 500, 1) >= 2 * 8 * 1000
    assert lib.hpcla_spmm_t_struct_i32(None, None, -1, 0, 0, None, None, None, None, 0, None) == -1
    assert lib.hpcla_spmm_t_f64_i32(None, None, None, None, 10, None, 16, 2, 16, None, 16, 0, None) == -1     # bad layout
    assert lib.hpcla_spmm_t_f64_i32(None, None, None, None, 10, None, 16, 0, 16, None, 15, 0, None) == -1     # ldw < m
    assert lib.hpcla_spmm_t_f64_i64(None, None, None, None, 0, None, 16, 0, 16, None, 16, 0, None) == 0      # nothing to do
    assert lib.hpcla_spmm_t_accumulate_f64(None, 4, None, 4, None, None, None, 0, 4, None) == 0
    assert lib.hpcla_spmm_t_accumulate_f64(None, 3, None, 4, None, None, None, 2, 4, None) == -1
