"""Worker for tests/test_gpu_gram.py: ONE process per rank (launch.spawn_ranks), ranks may share a GPU (the m x k sum then
goes through the communicator's peer window).  transpose(X) * Y through the host layer:
  * row partitions with an empty rank; m not divisible by the rank count; m * k <= 256;
  * integer-valued blocks: every slice bit-equal to the 1-rank product (= numpy's int64 product);
  * random blocks: within 1e-12 |X|^T |Y| of the 1-rank product; the gathered result bit-identical on every rank and on a
    second call; X'X exactly symmetric;
  * result partitions: rows = X.col_partition, columns = uniform_partition(k, nranks);
  * HPCLA_GRAM_MISMATCH=1: Y on another row partition than X (repartition_dense first; needs RCCL).
Exit code 0 = all passed on this rank."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")


def one_rank_product(hp, Xg, Yg):
    """the local product of the whole blocks, no communicator (the 1-rank result)"""
    import torch
    from hpcla_amd.vectors import current_stream_ptr, dptr
    n, m = Xg.shape
    k = Yg.shape[1]
    X = torch.from_numpy(np.ascontiguousarray(Xg)).cuda()
    Y = torch.from_numpy(np.ascontiguousarray(Yg)).cuda()
    C = torch.empty((m, k), dtype=torch.float64, device="cuda")
    work = torch.empty(max(1, hp._capi.load().hpcla_gram_work_bytes(n, m, k) // 8), dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_gram_f64", None, dptr(X), m, hp._capi.LAYOUT_ROW, dptr(Y), k, hp._capi.LAYOUT_ROW, n, m, k,
                  dptr(C), dptr(work), current_stream_ptr())
    torch.cuda.synchronize()
    return C.cpu().numpy()


def main():
    import torch
    import torch.distributed as dist
    import hpcla_amd as hp

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    backend = hp.backend_rocm_mpi(np.float64, np.int32)
    mismatch = os.environ.get("HPCLA_GRAM_MISMATCH") == "1"
    tag = f"[gram rank {rank}/{nranks} windows={backend.peer_windows} mismatch={mismatch}]"
    rng = np.random.default_rng(2024)                  # same stream on every rank: identical global blocks
    n = 100_003
    # the last rank holds no rows; the others split the rest unevenly
    px = np.array([0] + [(n * (r + 1)) // (nranks - 1) - 17 * r for r in range(nranks - 2)] + [n, n], dtype=np.int64)
    py = hp.uniform_partition(n, nranks) if mismatch else px
    for m, k in [(16, 16), (7, 5), (11, 11), (1, 3)]:
        for kind in ("int", "rand"):
            if kind == "int":
                Xg = rng.integers(-8, 9, size=(n, m)).astype(np.float64)
                Yg = rng.integers(-8, 9, size=(n, k)).astype(np.float64)
            else:
                Xg, Yg = rng.uniform(-1, 1, (n, m)), rng.uniform(-1, 1, (n, k))
            X = hp.HPCMatrix.from_global(Xg, backend, row_partition=px)
            Y = hp.HPCMatrix.from_global(Yg, backend, row_partition=py)
            ref = one_rank_product(hp, Xg, Yg)
            G = hp.transpose(X) @ Y
            assert np.array_equal(G.row_partition, X.col_partition), tag
            assert np.array_equal(G.row_partition, hp.uniform_partition(m, nranks)), tag
            assert np.array_equal(G.col_partition, hp.uniform_partition(k, nranks)), tag
            lo, hi = int(G.row_partition[rank]), int(G.row_partition[rank + 1])
            got = G.local_values()
            assert got.shape == (hi - lo, k), (tag, got.shape)
            if kind == "int":
                assert np.array_equal(ref, Xg.T @ Yg), tag
                assert np.array_equal(got, ref[lo:hi]), (f"{tag} {m}x{k} int: slice differs from the 1-rank product at "
                                                         f"{np.argwhere(got != ref[lo:hi])[:8].tolist()}: "
                                                         f"{got[got != ref[lo:hi]][:8]} vs {ref[lo:hi][got != ref[lo:hi]][:8]}")
            else:
                bound = 1e-12 * (np.abs(Xg).T @ np.abs(Yg))
                assert np.all(np.abs(got - ref[lo:hi]) <= bound[lo:hi]), f"{tag} {m}x{k} rand: outside the bound"
            full = G.gather()
            full2 = (hp.transpose(X) @ Y).gather()
            assert np.array_equal(full.view(np.uint64), full2.view(np.uint64)), f"{tag} {m}x{k}: two calls differ"
            every = [None] * nranks
            dist.all_gather_object(every, full.tobytes())
            assert all(e == every[0] for e in every), f"{tag} {m}x{k}: ranks disagree"
            if m == k and not mismatch:
                S = (hp.transpose(X) @ X).gather()
                assert np.array_equal(S, S.T), f"{tag} {m}: X'X not exactly symmetric"
                if kind == "int":
                    assert np.array_equal(S, Xg.T @ Xg), tag
    torch.cuda.synchronize()
    print(f"{tag} OK", file=sys.stderr)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
