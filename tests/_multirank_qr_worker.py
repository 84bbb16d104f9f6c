"""Worker for tests/test_gpu_qr.py::test_qr_across_ranks: ONE process per rank (launch.spawn_ranks), the ranks share the GPU.
``k = 16``, ``kappa = 1e12``, on explicit row partitions: one rank holds ``P F + 1`` rows (three levels of its own tree), one
holds 5 rows (fewer than ``k``: its triangle is zero-padded), and with three ranks one holds none (it still takes part in the
all-reduce).  Both orders of the large and the small rank are run.
  * orth and back of the gathered Q within 16 k eps (tests/_qr_cases.py; numpy.linalg.qr asserted within them too);
  * R well-formed and bit-identical on every rank; a second call gives the same bits of Q and R;
  * hp.lstsq on a consistent system at kappa = 1e3: ||c - c0|| / ||c0|| <= 10 kappa eps, rnorm <= 64 eps ||b||, c and rnorm
    bit-identical on every rank.  b is given on X's row partition: ranks that share a GPU have no RCCL communicator, which the
    repartition of a vector needs.
Exit code 0 = all passed on this rank."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main():
    import torch
    import torch.distributed as dist
    import hpcla_amd as hp
    from tests import _qr_cases as qc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[qr rank {rank}/{nranks}]"
    lib = hp._capi.load()
    k = 16
    big, small = lib.hpcla_qr_panel_rows() * lib.hpcla_qr_fan(k) + 1, 5
    n = big + small

    def same_on_every_rank(arr, what):
        mine = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64).reshape(-1).copy())
        every = [torch.empty_like(mine) for _ in range(nranks)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e.view(torch.int64), mine.view(torch.int64)) for e in every), (tag, what)

    parts = {"large first": [0, big, n], "small first": [0, small, n]}
    X = qc.make(n, k, 1e12, 3)
    Qn, Rn = np.linalg.qr(X)
    assert qc.orth(Qn) <= qc.limit(k) and qc.back(Qn, Rn, X) <= qc.limit(k)
    Xl = qc.make(n, k, 1e3, 4)
    c0 = np.random.default_rng(5).standard_normal(k)
    b = Xl @ c0
    for label, offsets in parts.items():
        part = np.array(offsets + [n] * (nranks + 1 - len(offsets)), dtype=np.int64)     # a third rank holds no rows
        Xh = hp.HPCMatrix.from_global(X, backend, row_partition=part)
        Q, R = hp.qr(Xh)
        assert Q.local_values().shape == (int(part[rank + 1] - part[rank]), k), tag
        assert np.array_equal(Q.row_partition, part) and np.array_equal(Q.col_partition, Xh.col_partition), tag
        Qg = Q.gather()
        o, bk = qc.orth(Qg), qc.back(Qg, R, X)
        print(f"{tag} {label}: orth {o / qc.EPS:.1f} eps, back {bk / qc.EPS:.1f} eps, limit {16 * k} eps", file=sys.stderr)
        assert o <= qc.limit(k) and bk <= qc.limit(k), (tag, label, o, bk)
        qc.check_r_shape(R, k)
        same_on_every_rank(R, "R")
        Q2, R2 = hp.qr(Xh)
        assert np.array_equal(R2.view(np.int64), R.view(np.int64)), (tag, label)
        assert np.array_equal(Q2.local_values().view(np.int64), Q.local_values().view(np.int64)), (tag, label)
        assert np.array_equal(hp.qr(Xh, mode="r").view(np.int64), R.view(np.int64)), (tag, label)

        Xlh = hp.HPCMatrix.from_global(Xl, backend, row_partition=part)
        c, rnorm = hp.lstsq(Xlh, hp.HPCVector.from_global(b, backend, partition=part))
        assert np.array_equal(c.partition, Xlh.col_partition), tag
        cg = c.gather()
        err = np.linalg.norm(cg - c0) / np.linalg.norm(c0)
        print(f"{tag} {label}: lstsq error {err:.1e} (limit {10 * 1e3 * qc.EPS:.1e}), rnorm / ||b|| {rnorm / np.linalg.norm(b):.1e}",
              file=sys.stderr)
        assert err <= 10 * 1e3 * qc.EPS and rnorm <= 64 * qc.EPS * np.linalg.norm(b), (tag, label, err, rnorm)
        same_on_every_rank(np.concatenate([cg, [rnorm]]), "lstsq")
        torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
