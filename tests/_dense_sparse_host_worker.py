"""Worker for tests/test_dense_sparse_host.py: one process per rank, gloo, CPU only.  A numpy executor of the host plans
of transpose(X) * A and X * A (transpose.HostSpmmTPlan, transpose.DenseTransposeLists), driven through the real comm_*
primitives:
  * local partial sums over the split column space (own columns, then the ghost segments), in ascending row order;
  * the reverse halo: ghost segments back to their owners, the owner's rows = own partial + peers in ascending rank;
  * copy(transpose(.)) block ranges and the result partitions;
integer inputs must reproduce X^T A and X A exactly.  Mutations (a reverse segment dropped, a peer's partial added twice)
must change the result on some rank.  Exit code 0 = all passed on this rank."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def local_partials(rowptr, split, vals, Xloc, ncols_split):
    W = np.zeros((ncols_split, Xloc.shape[1]), dtype=np.int64)
    for r in range(len(rowptr) - 1):                       # ascending rows: each column's sum in CSC order
        for e in range(rowptr[r], rowptr[r + 1]):
            W[split[e]] += vals[e] * Xloc[r]
    return W


def reverse_halo(B, comm, h, W, mutate=None):
    m = W.shape[1]
    sends = [W[o:o + c].ravel() for o, c in zip(h.back_offsets, h.back_counts)]
    if mutate == "drop" and sends:
        sends[-1] = np.zeros_like(sends[-1])              # one reverse segment lost
    got = B.comm_exchange_arrays(comm, h.back_ranks, sends, h.from_ranks, [c * m for c in h.from_counts], np.float64)
    R = np.concatenate([g.reshape(-1, m) for g in got]).astype(np.int64) if got else np.zeros((0, m), dtype=np.int64)
    assert R.shape[0] == h.n_recv
    V = W[:h.n_own].copy()
    for u, row in enumerate(h.acc_rows):
        for t in range(h.acc_ptr[u], h.acc_ptr[u + 1]):
            V[row] += R[h.acc_pos[t]]
        if mutate == "twice" and h.acc_ptr[u + 1] > h.acc_ptr[u]:
            V[row] += R[h.acc_pos[h.acc_ptr[u]]]           # a peer's partial added a second time
    return V


def block_transpose(B, comm, L, M):
    """this rank's rows of M^T (M: the local rows on P, m columns) through the DenseTransposeLists L"""
    T = np.ascontiguousarray(M.T).ravel()                  # m x n_me, row-major
    assert T.size == L.n_me * M.shape[1]
    got = B.comm_exchange_arrays(comm, L.send_ranks, [T[o:o + c] for o, c in zip(L.send_offsets, L.send_counts)],
                                 L.recv_ranks, L.recv_counts, np.float64)
    buf = np.full(L.n_buf, -999, dtype=np.int64)
    for off, g in zip(L.recv_offsets, got):
        buf[off:off + len(g)] = g.astype(np.int64)
    buf[L.local_dst:L.local_dst + L.local_count] = T[L.local_src:L.local_src + L.local_count]
    out = np.full((L.q_me, L.ncols), -999, dtype=np.int64)
    for _q, off, n_q, c0 in L.blocks:
        out[:, c0:c0 + n_q] = buf[off:off + L.q_me * n_q].reshape(L.q_me, n_q)
    return out


def main():
    import scipy.sparse as sp
    import torch.distributed as dist
    import hpcla_amd as hp
    from hpcla_amd import backends as B
    from hpcla_amd.sparse import _compress_columns

    dist.init_process_group("gloo")
    rank, nranks = dist.get_rank(), dist.get_world_size()
    comm = hp.CommTorch()
    rng = np.random.default_rng(77)                        # same stream on every rank: identical global inputs
    checks = 0
    for p, n, m, dens in [(97, 61, 5, 0.08), (400, 400, 16, 0.01), (50, 300, 3, 0.05), (300, 40, 7, 0.1)]:
        S = sp.random(p, n, density=dens, format="csr", random_state=np.random.RandomState(int(rng.integers(1 << 30))),
                      data_rvs=lambda k: rng.integers(-9, 10, size=k).astype(np.float64))
        S.sort_indices()
        Ad = S.toarray().astype(np.int64)
        Xg = rng.integers(-8, 9, size=(p, m)).astype(np.int64)        # transpose(X) * A: X is p x m
        Zg = rng.integers(-8, 9, size=(m, p)).astype(np.int64)        # X * A: Z is m x p
        # A's rows: the last rank empty when there are more than two ranks
        if nranks > 2:
            pa = np.array([0] + [(p * (r + 1)) // (nranks - 1) for r in range(nranks - 1)] + [p], dtype=np.int64)
        else:
            pa = np.array([0, p // 3, p], dtype=np.int64)
        pc = hp.uniform_partition(n, nranks)
        qm = np.array([0] + [min(m, 2 * (r + 1)) for r in range(nranks - 1)] + [m], dtype=np.int64)   # X.col_partition
        qm = np.maximum.accumulate(qm)
        lo, hi = int(pa[rank]), int(pa[rank + 1])
        loc = S[lo:hi]
        col_indices, colval = _compress_columns(loc.indices.astype(np.int64), n, np.int32)
        h = hp.HostSpmmTPlan(col_indices, pc, comm)
        assert h.n_own == int(pc[rank + 1] - pc[rank]) and h.ncols_split == h.n_own + h.n_ghost
        split = h.cmap[colval.astype(np.int64)]
        own_cols = np.arange(int(pc[rank]), int(pc[rank + 1]))
        for kind in ("XtA", "XA"):
            if kind == "XtA":
                Xloc, Q, want = Xg[lo:hi], qm, Xg.T @ Ad
            else:
                # copy(transpose(Z)) straight onto A's row partition; Z's rows on uniform_partition(m)
                pz = hp.uniform_partition(m, nranks)
                Lz = hp.DenseTransposeLists(pz, pa, rank)
                Xloc = block_transpose(B, comm, Lz, Zg[int(pz[rank]):int(pz[rank + 1])])
                assert Xloc.shape == (hi - lo, m) and np.array_equal(Xloc, Zg.T[lo:hi])
                Q, want = pz, Zg @ Ad
            W = local_partials(loc.indptr, split, loc.data.astype(np.int64), Xloc, h.ncols_split)
            V = reverse_halo(B, comm, h, W)
            assert np.array_equal(V, want[:, own_cols].T), f"reverse halo, rank {rank}"
            L = hp.DenseTransposeLists(pc, Q, rank)
            C = block_transpose(B, comm, L, V)
            assert C.shape == (int(Q[rank + 1] - Q[rank]), n)
            assert np.array_equal(C, want[int(Q[rank]):int(Q[rank + 1])]), f"{kind} result rows, rank {rank}"
            checks += 1
            # the executor must go red when a nonzero partial travels back wrongly
            last = np.abs(W[h.back_offsets[-1]:h.back_offsets[-1] + h.back_counts[-1]]).sum() if h.back_ranks else 0
            travelled = B.comm_allgather(comm, np.array([last], dtype=np.int64)).sum()
            for mut in ("drop", "twice"):
                Vm = reverse_halo(B, comm, h, W, mutate=mut)
                differs = B.comm_allgather(comm, np.array([0 if np.array_equal(Vm, V) else 1], dtype=np.int64))
                if travelled > 0:
                    assert differs.sum() > 0, f"mutation {mut} went unnoticed"
    dist.barrier()
    dist.destroy_process_group()
    print(f"rank {rank}: {checks} products: OK")


if __name__ == "__main__":
    main()
