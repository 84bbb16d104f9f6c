"""Worker for tests/test_gpu_packed_edges.py::test_packed_interior_across_ranks: ONE process per rank (launch.spawn_ranks), the
ranks share the GPU.  The periodic 9-point (40 x 32 R) and 27-point (12 x 12 x 8 R) stencils of tests/_packed_cases.py, split
evenly by rows over R ranks: every rank holds whole row blocks of 2304 / 6912 entries (two / four passes of the packed kernel)
whose columns are all its own -- the packed interior -- and, at both ends of its range, blocks with columns of its neighbours
(the wrap makes the first and the last rank neighbours too), which stay on the CSR kernel behind the exchange.
  * enable_packed is True on every rank and leaves a handle; the interior list is the one numpy derives from the columns;
  * A @ x, repeated mul_ and mul_dot_'s y have the bits of this rank's rows of the ONE-rank oracle product;
  * mul_dot_'s scalar is within RTOL_RED * |x|.|y| of the oracle's global dot and has the same bits on every rank;
  * no push / wait timed out.
A failed check ends the process at once (exit code 1, nothing more is started on the GPU); spawn_ranks then stops the other
ranks.  Exit code 0 = all passed on this rank."""
import os
import sys
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

RTOL_RED = 1e-12


def main():
    import torch
    import torch.distributed as dist
    import hpcla_amd as hp
    from oracle import oracle as orc
    import _packed_cases as pc

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    os.environ.pop("HPCLA_SPMV_PACKED", None)
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    tag = f"[packed rank {rank}/{nranks}]"

    for name, dims, passes in (("stencil9", (40, 32 * nranks), 2), ("stencil27", (12, 12, 8 * nranks), 4)):
        gen = getattr(pc, name)
        n = int(np.prod(dims))
        part = orc.uniform_partition(n, nranks)
        lo, hi = int(part[rank]), int(part[rank + 1])
        assert hi - lo == n // nranks and (hi - lo) > 4 * pc.RPB, (tag, name, lo, hi)
        full = gen(*dims)
        xg = orc.fill_uniform(0, n, orc.SEED_X) - 0.5
        want_all = orc.spmv(full[0].astype(np.int32), full[1].astype(np.int32), full[2], xg)     # the one-rank product
        want = want_all[lo:hi]
        rowptr, col, vals = gen(*dims, lo, hi)
        A = hp.HPCSparseMatrix_local(rowptr, col, vals, n, backend)
        x = hp.HPCVector.from_global(xg, backend, partition=part)
        plan = hp.get_vector_plan(A, x)
        assert plan.has_halo and plan.n_interior > 0 and plan.n_boundary > 0, (tag, name, plan.n_interior, plan.n_boundary)
        # the interior blocks, independently of the device: no column of another rank; each takes `passes` passes
        own = (col >= lo) & (col < hi)
        nblk = pc.n_blocks(hi - lo)
        interior = [b for b in range(nblk) if own[rowptr[pc.RPB * b]:rowptr[min(pc.RPB * b + pc.RPB, hi - lo)]].all()]
        assert np.array_equal(plan.interior.cpu().numpy(), interior) and len(interior) >= 2, (tag, name, interior)
        assert all(pc.n_passes(rowptr, b) == passes for b in interior), (tag, name)
        assert pc.eligible_np(rowptr, np.where(own, col - lo, hi - lo), hi - lo, blocks=interior), (tag, name)

        assert A.enable_packed(x) is True, (tag, name, A.packed_reason)
        assert A._packed.get(plan.key) is not None and A._packed_for(plan) is not None, (tag, name)
        y = A @ x
        for _ in range(3):
            hp.mul_(y, A, x)
        torch.cuda.synchronize()
        got = y.local_values().copy()
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), \
            f"{tag} {name}: A @ x differs from the one-rank oracle in {int((got != want).sum())} rows"
        yd = x.similar()
        yd.v.fill_(float("nan"))
        out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        hp.mul_dot_(yd, A, x, out)
        torch.cuda.synchronize()
        got = yd.local_values().copy()
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), f"{tag} {name}: mul_dot_ y differs"
        ref, bound = orc.dot([xg], [want_all]), RTOL_RED * float(np.abs(xg) @ np.abs(want_all))
        print(f"{tag} {name}: x.Ax {out.item()!r} reference {ref!r} bound {bound:.3e}", file=sys.stderr)
        assert abs(out.item() - ref) <= bound, (tag, name, out.item(), ref)
        mine = out.cpu().view(torch.int64)
        every = [torch.empty_like(mine) for _ in range(nranks)]
        dist.all_gather(every, mine)
        assert all(torch.equal(e, mine) for e in every), (tag, name, "the scalar differs between ranks")
        assert not plan.timed_out(), f"{tag} {name}: a push / wait timed out"
        A.disable_packed()
        hp.mul_(y, A, x)
        torch.cuda.synchronize()
        assert np.array_equal(y.local_values().view(np.int64), want.view(np.int64)), f"{tag} {name}: CSR differs"
    hp.clear_plan_cache()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except BaseException:                       # a failed check: say so and end here, with nothing more started on the GPU
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
