"""GPU worker of tests/test_gpu_block_patterns.py (one process per rank, ranks may share a GPU: the push transport): a 2-D
Poisson slab per rank through the host layer.  Interior row blocks run in the pattern form (columns and row bounds from the
plan's table), boundary blocks (ghost columns) on Int32; A*x, repeated mul!, dependent steps and mul_dot_ must have the bits
of the per-rank oracle pipeline and of the same calls under HPCLA_BLOCK_PATTERNS=0 (streamed 16-bit columns).  The pattern
of tests/_narrow_cols_rank_worker.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def main():
    import torch
    import torch.distributed as dist
    import hpcla_amd as hp
    from oracle import oracle as orc
    from _block_patterns_cases import model_table
    from hpcla_amd.sparse import block_patterns_info

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    os.environ.pop("HPCLA_NARROW_COLS", None)
    os.environ.pop("HPCLA_BLOCK_PATTERNS", None)
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[rank {rank}/{nranks} windows={backend.peer_windows}]"

    nx, ny = 512, 9 * nranks + 2                   # ~9 grid lines = 18 row blocks per rank, 2 of them at each inner edge
    n = nx * ny
    rp = orc.uniform_partition(n, nranks)
    lo, hi = int(rp[rank]), int(rp[rank + 1])
    rows = orc.poisson2d_rows(nx, ny, lo, hi)
    ci, cv = orc.compress_columns(rows)
    xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.25
    want = orc.spmv(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, xg[ci])

    # dependent steps of the whole matrix on the host (every rank computes all ranks' parts: the oracle pipeline)
    full = orc.poisson2d_rows(nx, ny, 0, n)
    xs_ref = xg.copy()
    for _ in range(6):
        xs_ref = orc.spmv(full.rowptr.astype(np.int32), full.colidx.astype(np.int32), full.vals, xs_ref) * 0.125

    results = {}
    for leg in ("patterns", "streamed"):
        if leg == "streamed":
            os.environ["HPCLA_BLOCK_PATTERNS"] = "0"
        A = hp.HPCSparseMatrix_local(rows.rowptr, rows.colidx, rows.vals, n, backend)
        x = hp.HPCVector.from_global(xg, backend, partition=rp)
        plan = hp.get_vector_plan(A, x)
        assert plan.has_halo and plan.push, f"{tag}: push transport not attached"
        assert plan.n_interior > 0 and plan.n_boundary > 0, (tag, plan.n_interior, plan.n_boundary)
        assert plan.cols16 is not None, f"{tag}: the slab's interior blocks are eligible"
        if leg == "patterns":
            # what the table must hold, from the host arrays: the interior blocks' patterns over LOCAL column offsets
            blocks = plan.interior.cpu().numpy()
            own = (rows.colidx >= lo) & (rows.colidx < hi)
            model = model_table(rows.rowptr, np.where(own, rows.colidx - lo, hi - lo), blocks=blocks)
            assert plan.patterns is not None and block_patterns_info(plan.patterns) == model, (tag, model)
            assert model["patterned"] == len(blocks)
        else:
            assert plan.patterns is None
        y = A @ x
        for _ in range(4):
            hp.mul_(y, A, x)
        torch.cuda.synchronize()
        got = y.local_values().copy()
        assert np.array_equal(got, want), f"{tag} {leg}: A*x differs in {int((got != want).sum())} rows"
        xs, ys = hp.HPCVector.from_global(xg, backend, partition=rp), x.similar()
        for _ in range(6):                          # x_{k+1} = A x_k / 8 with no host sync in between: ghost buffers alternate
            hp.mul_(ys, A, xs)
            xs.v.copy_(ys.v)
            xs.v.mul_(0.125)
        torch.cuda.synchronize()
        assert np.array_equal(xs.local_values(), xs_ref[lo:hi]), f"{tag} {leg}: dependent steps differ"
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        yd = x.similar()
        hp.mul_dot_(yd, A, x, out)
        torch.cuda.synchronize()
        assert np.array_equal(yd.local_values(), want), f"{tag} {leg}: mul_dot_ y differs"
        assert not plan.timed_out(), f"{tag} {leg}: a push / wait timed out"
        results[leg] = (got, out.cpu().numpy().copy())
    assert np.array_equal(results["patterns"][0], results["streamed"][0])
    assert np.array_equal(results["patterns"][1].view(np.int64), results["streamed"][1].view(np.int64)), f"{tag}: p.Ap bits differ"
    os.environ.pop("HPCLA_BLOCK_PATTERNS", None)
    hp.clear_plan_cache()
    dist.barrier()
    if rank == 0:
        print("block patterns rank worker OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
