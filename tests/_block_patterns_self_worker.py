"""GPU worker of tests/test_gpu_block_patterns.py: the distributed SpMV with a PATTERNED interior under each ordering
(HPCLA_HALO_MODE = serial / overlap / push) on ONE GPU, with a one-rank communicator that exchanges with itself
(HPCLA_FORCE_RCCL=1) -- the problems of tests/_narrow_cols_self_worker.py.  Interior blocks go through the pattern form of
the narrow kernel (a contiguous run by its base, and -- second problem -- a scattered list), boundary blocks through the
Int32 kernel; the table is created over the interior blocks only (by list, and for the run also by base and length)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import hpcla_amd as hp
    from hpcla_amd.backends import attach_halo_windows
    from oracle import oracle as orc
    from _narrow_cols_cases import eligible_np
    from _block_patterns_cases import model_table
    from hpcla_amd.sparse import block_patterns_info

    assert os.environ.get("HPCLA_FORCE_RCCL") == "1"
    push = os.environ.get("HPCLA_HALO_MODE", "") == "push"
    backend = hp.backend_rocm_serial(np.float64, np.int32)
    assert backend.peer_windows
    capi = hp._capi
    lib = capi.load()
    s = torch.cuda.current_stream().cuda_stream
    rpb = lib.hpcla_spmv_rows_per_block()

    def problem(nx, ny, ghost_rows_of):
        """Local rows of a grid one line taller than the slab: the line above is fetched through the halo from this rank's own
        rows `ghost_rows_of(g)`."""
        nloc = nx * ny
        rows = orc.poisson2d_rows(nx, ny + 1, 0, nloc)
        ci, cv = orc.compress_columns(rows)
        assert int((ci >= nloc).sum()) == nx
        xg = orc.fill_uniform(0, nloc, 44) - 0.5
        send_idx = ghost_rows_of(np.arange(nx))
        x_ext = np.concatenate([xg, xg[send_idx]])
        return nloc, rows, ci[cv], xg, send_idx, x_ext

    def run(nloc, rowptr, col_split, vals, xg, send_idx, x_ext, expect_contig):
        nnz = len(col_split)
        want = orc.spmv(rowptr.astype(np.int32), col_split.astype(np.int32), vals, x_ext)
        plan = ctypes.c_void_p()
        d_idx = torch.from_numpy(send_idx.astype(np.int32)).cuda()
        ranks = (ctypes.c_int32 * 1)(0)
        counts = (ctypes.c_int64 * 1)(len(send_idx))
        torch.cuda.synchronize()
        capi.check("create", lib.hpcla_halo_plan_create(ctypes.byref(plan), backend.rccl, 1, ranks, counts,
                                                       d_idx.data_ptr(), 0, 1, ranks, counts, 1))
        assert attach_halo_windows(backend, plan) == push
        d_rp = torch.from_numpy(rowptr.astype(np.int32)).cuda()
        d_cv = torch.from_numpy(col_split.astype(np.int32)).cuda()
        vbuf = torch.full((nnz + 64,), float("nan"), dtype=torch.float64, device="cuda")     # nzval ends inside a NaN guard
        vbuf[:nnz] = torch.from_numpy(vals).cuda()
        d_nz = vbuf[:nnz]
        d_x = torch.from_numpy(xg).cuda()
        nblk = (nloc + rpb - 1) // rpb
        flags = torch.empty(nblk, dtype=torch.int32, device="cuda")
        capi.call("hpcla_classify_blocks_i32", d_rp.data_ptr(), d_cv.data_ptr(), nloc, 0, nloc, rpb, flags.data_ptr(), s)
        interior = torch.nonzero(flags == 0).flatten().to(torch.int32).contiguous()
        boundary = torch.nonzero(flags != 0).flatten().to(torch.int32).contiguous()
        ib = interior.cpu().numpy()
        assert len(ib) > 0 and boundary.numel() > 0
        assert (int(ib[-1]) - int(ib[0]) + 1 == len(ib)) == expect_contig
        assert eligible_np(rowptr, col_split, nloc, blocks=ib) and not eligible_np(rowptr, col_split, nloc)
        c16 = torch.empty(lib.hpcla_cols16_padded_len(nnz), dtype=torch.int16, device="cuda")
        bad = torch.ones(1, dtype=torch.int32, device="cuda")
        capi.call("hpcla_cols16_encode_i32", d_rp.data_ptr(), d_cv.data_ptr(), nloc, nnz, nloc, 0, interior.data_ptr(),
                  interior.numel(), c16.data_ptr(), bad.data_ptr(), s)
        assert int(bad.item()) == 0, "the interior blocks are eligible"
        capi.call("hpcla_cols16_encode_i32", d_rp.data_ptr(), d_cv.data_ptr(), nloc, nnz, nloc, 0, None, 0,
                  torch.empty_like(c16).data_ptr(), bad.data_ptr(), s)
        assert int(bad.item()) != 0, "boundary blocks hold ghost columns: all blocks together are not eligible"
        # the table over the interior blocks: what the numpy model predicts, whichever way the blocks are named
        handles = [ctypes.c_void_p()]
        capi.call("hpcla_block_patterns_create_i32", ctypes.byref(handles[0]), d_rp.data_ptr(), c16.data_ptr(), nloc, nnz, 0,
                  interior.data_ptr(), -1, interior.numel(), 0, s)
        if expect_contig:
            handles.append(ctypes.c_void_p())
            capi.call("hpcla_block_patterns_create_i32", ctypes.byref(handles[1]), d_rp.data_ptr(), c16.data_ptr(), nloc, nnz, 0,
                      None, int(ib[0]), len(ib), 0, s)
        model = model_table(rowptr, col_split, blocks=ib)
        assert model is not None and model["patterned"] > len(ib) // 2
        for h in handles:
            assert h and block_patterns_info(h) == model, (block_patterns_info(h), model)
        pat = handles[-1]
        y = torch.full((nloc,), float("nan"), dtype=torch.float64, device="cuda")
        y32 = torch.full((nloc,), float("nan"), dtype=torch.float64, device="cuda")
        for rep in range(5):                       # repeated use: both ghost buffers, WAR ordering
            capi.call("hpcla_spmv_dist_patterns_f64_i32", plan, d_rp.data_ptr(), d_cv.data_ptr(), c16.data_ptr(), pat, d_nz.data_ptr(),
                      d_x.data_ptr(), nloc, y.data_ptr(), nloc, nnz, 0, interior.data_ptr(), interior.numel(),
                      boundary.data_ptr(), boundary.numel(), s)
        capi.call("hpcla_spmv_dist_f64_i32", plan, d_rp.data_ptr(), d_cv.data_ptr(), d_nz.data_ptr(), d_x.data_ptr(), nloc,
                  y32.data_ptr(), nloc, nnz, 0, interior.data_ptr(), interior.numel(), boundary.data_ptr(), boundary.numel(), s)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        assert np.array_equal(got, want), f"patterned distributed SpMV differs in {int((got != want).sum())} rows"
        assert np.array_equal(y32.cpu().numpy(), want)
        work = torch.empty(lib.hpcla_spmv_dot_work_bytes(nloc) // 8 + 1, dtype=torch.float64, device="cuda")
        dots = []
        for fn, extra in (("hpcla_spmv_dist_dot_patterns_f64_i32", (c16.data_ptr(), pat)),
                          ("hpcla_spmv_dist_dot_cols16_f64_i32", (c16.data_ptr(),)), ("hpcla_spmv_dist_dot_f64_i32", ())):
            yd = torch.full((nloc,), float("nan"), dtype=torch.float64, device="cuda")
            out = torch.zeros(1, dtype=torch.float64, device="cuda")
            for rep in range(2):
                capi.call(fn, plan, backend.rccl, d_rp.data_ptr(), d_cv.data_ptr(), *extra, d_nz.data_ptr(), d_x.data_ptr(), nloc,
                          yd.data_ptr(), nloc, nnz, 0, interior.data_ptr(), interior.numel(), boundary.data_ptr(),
                          boundary.numel(), out.data_ptr(), work.data_ptr(), s)
            torch.cuda.synchronize()
            assert np.array_equal(yd.cpu().numpy(), want), fn
            dots.append(out.cpu().numpy().copy())
        assert np.array_equal(dots[0].view(np.int64), dots[1].view(np.int64)), "x.y differs in bits between table and stream"
        assert np.array_equal(dots[0].view(np.int64), dots[2].view(np.int64)), "x.y differs in bits between the column widths"
        # a NULL handle is exactly the cols16 entry point
        y0 = torch.full((nloc,), float("nan"), dtype=torch.float64, device="cuda")
        capi.call("hpcla_spmv_dist_patterns_f64_i32", plan, d_rp.data_ptr(), d_cv.data_ptr(), c16.data_ptr(), None, d_nz.data_ptr(),
                  d_x.data_ptr(), nloc, y0.data_ptr(), nloc, nnz, 0, interior.data_ptr(), interior.numel(),
                  boundary.data_ptr(), boundary.numel(), s)
        torch.cuda.synchronize()
        assert np.array_equal(y0.cpu().numpy(), want)
        st = ctypes.c_int(0)
        capi.call("hpcla_halo_status", plan, ctypes.byref(st))
        assert st.value == 0, "push / wait timed out"
        capi.call("hpcla_halo_plan_destroy", plan)
        for h in handles:
            capi.call("hpcla_block_patterns_destroy", h)

    # 1. the slab: ghosts are referenced by the last grid line only -> boundary blocks at the end, interior one contiguous run
    nx, ny = 512, 40
    nloc, rows, col_split, xg, send_idx, x_ext = problem(nx, ny, lambda g: g + 3 * nx)
    run(nloc, rows.rowptr, col_split, rows.vals, xg, send_idx, x_ext, expect_contig=True)

    # 2. the same slab with the ghost line ALSO referenced from rows in the middle (their last entry's column is replaced by
    #    a ghost column, keeping every row ascending: ghosts are the largest columns): the interior is a list with holes
    col2 = col_split.copy()
    rp = rows.rowptr
    for r in (5 * rpb + 17, 11 * rpb + 255, 30 * rpb):
        last = rp[r + 1] - 1
        assert col2[last] < nloc
        col2[last] = nloc + (r % nx)
    run(nloc, rp, col2, rows.vals, xg, send_idx, x_ext, expect_contig=False)
    print("patterned self-exchange OK")


if __name__ == "__main__":
    main()
