"""Child process of tests/test_gpu_spmv_sweep.py: the host-layer products of the 64 x 64 5-point matrix in a fresh process,
under whatever HPCLA_SPMV_SWEEP the parent set.  Writes OUT.npz: y of four hp.mul_ calls with a pattern-table plan (y_pat)
and under HPCLA_BLOCK_PATTERNS=0 (y_nopat), and the sweep direction the library reported after each call."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def products(hp, orc, backend, patterns: bool):
    """(four y arrays, four reported directions, the plan) of hp.mul_ on the 64 x 64 matrix."""
    N = 64
    n = N * N
    rows = orc.poisson2d_rows(N, N, 0, n)
    xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.5
    if patterns:
        os.environ.pop("HPCLA_BLOCK_PATTERNS", None)
    else:
        os.environ["HPCLA_BLOCK_PATTERNS"] = "0"
    try:
        A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, backend)
        x = hp.HPCVector.from_global(xg, backend)
        plan = hp.get_vector_plan(A, x)
        y = x.similar()
        ys, dirs = [], []
        rev = ctypes.c_int(-1)
        for _ in range(4):
            y.v.fill_(float("nan"))
            hp.mul_(y, A, x)
            hp._capi.call("hpcla_spmv_last_sweep", ctypes.byref(rev))
            ys.append(y.local_values().copy())
            dirs.append(int(rev.value))
    finally:
        os.environ.pop("HPCLA_BLOCK_PATTERNS", None)
    return ys, dirs, plan


def main() -> int:
    import hpcla_amd as hp
    from oracle import oracle as orc
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    yp, dp, _ = products(hp, orc, backend, True)
    yn, dn, _ = products(hp, orc, backend, False)
    np.savez(sys.argv[1], y_pat=np.stack(yp), y_nopat=np.stack(yn), dirs_pat=np.array(dp), dirs_nopat=np.array(dn))
    hp.clear_plan_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
