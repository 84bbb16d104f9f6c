"""Worker for tests/test_gpu_amg_nonsym.py::test_nonsymmetric_aggregation_across_ranks: ONE process per rank (launch.spawn_ranks),
the ranks share the GPU.  ``amg.aggregate_level(A, theta, symmetric=False)`` -- the rank-local part of a level's setup, which
exchanges sizes only -- on the uniform partition of the purely upwind 33 x 31 stencil (a structurally nonsymmetric pattern whose
couplings cross the rank boundaries one way only) and of the 24 x 20 convection-diffusion stencil: each rank's aggregate ids,
its root count and the coarse partition equal the blocked restatement of tests/_amg_nonsym_cases.py (ghost columns stay out of
E and of E^T, so aggregates never cross a rank); a non-bool ``symmetric`` raises on every rank; ``hp.amg(A, symmetric=False)``
itself is refused across ranks as the symmetric mode is.
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
    from tests import _amg_nonsym_cases as nc
    amg_mod = sys.modules[hp.amg.__module__]

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[amg nonsym rank {rank}/{nranks}]"

    def local_matrix(Ah, part):
        lo, hi = int(part[rank]), int(part[rank + 1])
        a, b_ = int(Ah.indptr[lo]), int(Ah.indptr[hi])
        return hp.HPCSparseMatrix_local(Ah.indptr[lo:hi + 1] - a, Ah.indices[a:b_], Ah.data[a:b_], Ah.shape[0], backend,
                                        col_partition=np.asarray(part, dtype=np.int64))

    for what, Ah, theta in (("upwind 33 x 31", nc.upwind(33, 31), 0.0), ("convection-diffusion 24 x 20", nc.convection_diffusion(24, 20), 0.0),
                            ("convection-diffusion 24 x 20, theta 0.25", nc.convection_diffusion(24, 20), 0.25)):
        part = hp.uniform_partition(Ah.shape[0], nranks)
        blocks = [int(v) for v in part]
        lo, hi = blocks[rank], blocks[rank + 1]
        agg, counts, _, rounds, _ = nc.aggregate(Ah, blocks, theta)
        lvl = amg_mod.aggregate_level(local_matrix(Ah, part), theta=theta, symmetric=False)
        assert np.array_equal(lvl.aggregates.cpu().numpy(), agg[lo:hi]), (tag, what)
        assert lvl.n_roots == int(counts[rank]), (tag, what)
        assert np.array_equal(lvl.coarse_partition, np.concatenate([[0], np.cumsum(counts)])), (tag, what)
        assert 1 <= lvl.rounds <= rounds, (tag, what)

    Ah = nc.upwind(33, 31)
    part = hp.uniform_partition(Ah.shape[0], nranks)
    try:
        amg_mod.aggregate_level(local_matrix(Ah, part), symmetric=0)
        raise AssertionError(tag + " no error")
    except TypeError as e:
        assert "symmetric" in str(e), (tag, str(e))
    try:
        hp.amg(local_matrix(Ah, part), symmetric=False)
        raise AssertionError(tag + " no refusal")
    except NotImplementedError as e:
        assert str(e).startswith("amg: one rank only"), (tag, str(e))

    torch.cuda.synchronize()
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
