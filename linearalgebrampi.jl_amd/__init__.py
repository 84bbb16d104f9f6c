"""linearalgebrampi.jl_amd -- MI355X-native DeviceROCm backend for the HPCLinearAlgebra.jl
(sloisel/LinearAlgebraMPI.jl) distributed SpMV / SpMM / CG hot path.

Layout
  csrc/              hand-written HIP kernels + the C ABI (include/hpcla_rocm.h) -> libhpcla_rocm.so
  _capi.py           ctypes binding of the C ABI (no fallback)
  backends.py        HPCBackend{T,Ti,Device,Comm,Solver}, DeviceROCm, comm_* primitives
  partition.py       uniform_partition, structural hashes
  vectors.py         HPCVector, dot, norm, fused updates
  sparse.py          HPCSparseMatrix, VectorPlan (host lists + device plan), A*x, mul!
  dense.py           HPCMatrix, dense A*x and transpose(A)*x, transpose(X)*Y, X*A and transpose(X)*A
  spmm_plans.py      A*B for a sparse A and a dense B (SpMM): exchange entries, sequential and panel orders
  cg.py              fixed-iteration CG harness; cg(): the converging solver (Jacobi or FSAI preconditioner, device-side stop)
  krylov.py          what the chunked solvers below share: CGInfo, the history of pairs, argument rules, the chunk loop with its
                     16-byte read-back, the M of bicgstab() and gmres(); their host-side iteration loops are csrc/solvers.hip
  fsai.py            fsai(): the factorised sparse approximate inverse preconditioner G' G of an SPD A for cg(M=...): one small dense
                     Cholesky per row on the device (csrc/fsai.hip), applied as two SpMVs; rank-local couplings, <= 32 entries per row
  amg.py             amg(): the smoothed-aggregation multigrid preconditioner of an SPD A for cg(M=...): aggregation by a distance-2
                     independent set on the device (csrc/amg.hip), the hierarchy through spgemm and transpose, a symmetric
                     V(1,1) cycle on ordinary SpMVs; aggregates never cross ranks
  ilu.py             ilu0(): the fine-grained ILU(0) preconditioner of a nonsymmetric A for gmres(M=...) and bicgstab(M=...):
                     Chow-Patel sweeps build the factors, truncated Jacobi sweeps stand for the triangular solves (csrc/ilu.hip);
                     rank-local couplings, no fill, no kernel that waits
  bicgstab.py        bicgstab(): BiCGStab for nonsymmetric A, the same device-side stop (csrc/vecops.hip, bicg_* kernels)
  gmres.py           gmres(): restarted GMRES(m), fused twice-applied Gram-Schmidt, the same device-side stop (gmres_* kernels)
  lsqr.py            lsqr(): least squares for rectangular A on A and its materialised transpose, damped form, two stop rules
                     on the device (lsqr_* kernels)
  minres.py          minres(): MINRES for symmetric indefinite A, diagonal preconditioner, the same device-side stop in the M norm
                     (minres_* kernels)
  eigsh.py           eigsh(): extreme eigenpairs of a symmetric A by thick-restart Lanczos on the GMRES kernels; the restart
                     rotates the basis in place in one pass (csrc/eigsh.hip)
  lobpcg.py          lobpcg(): the k <= 16 smallest or largest eigenpairs with their multiplicities by LOBPCG (optionally
                     Jacobi-preconditioned), of A or of the pencil A x = lambda B x (B sparse SPD, or positive weights): the SpMM,
                     one Gram pass, a host Rayleigh-Ritz, the block kernels of csrc/lobpcg.hip
  svds.py            svds(): the largest singular triplets of a rectangular A by thick-restart Golub-Kahan bidiagonalisation on A
                     and its materialised transpose: the GMRES kernels on two bases, a small step of its own (svds_* kernels), the
                     eigensolver's rotate for both restarts
  qr.py              qr(), lstsq(): tall-skinny Householder QR (TSQR) of a dense HPCMatrix of k <= 32 columns, Q formed from the
                     stored reflectors, and dense least squares through the augmented block [X b] (csrc/qr.hip)
  assemble.py        assembly_plan(), sparse_from_coo(): Julia's sparse(I, J, V, m, n) on the device with a reusable structure: a
                     stable sort and an inverted index once per (I, J), then one kernel per new V that sums every entry's
                     contributions in a fixed order without atomics (csrc/assemble.hip); off-rank triplets travel by a halo plan
  indexing.py        v[a:b], X[r, c], A[r, c], A[:, k], diag(A) and SubmatrixPlan (csrc/submatrix.hip)
  select.py          select(), take(), put_(), selection_plan(), index_plan(): A[rows, cols], v[idx] and v[idx] = src for index
                     LISTS (Dirichlet elimination, symmetric permutations, non-contiguous blocks): a column look-up, two scans
                     and a per-row rank-and-fill that keeps columns ascending (csrc/select.hip); off-rank vector entries
                     travel by a halo plan
  rcm.py             rcm(), bandwidth(): the reverse Cuthill-McKee ordering of a rank's owned block as an index list for select(),
                     take() and put_(): ties broken by (degree, index), levels walked by one workgroup in LDS while they are
                     narrow and device-wide otherwise, one integer state array under atomic min (csrc/rcm.hip); rank-local
  transpose.py matmat.py addition.py repartition.py   the SURVEY 8f "next" rows and their plans

The directory name contains a dot, so it is imported through the top-level alias module
``hpcla_amd`` (``import hpcla_amd as hp``).
"""
from . import _capi
from .backends import (AbstractComm, AbstractDevice, CommSerial, CommTorch, DeviceCPU, DeviceROCm, HPCBackend,
                       SolverNone, assert_backends_compatible, backend_rocm_mpi,
                       backend_rocm_serial, backends_compatible, comm_exchange_arrays, comm_rank, comm_size,
                       cpu_version, eltype_backend, indextype_backend)
from .partition import (compute_partition_hash, compute_structural_hash, local_window, owner_of, subpartition,
                        uniform_partition)
from .vectors import HPCVector, HPCVector_local, cg_direction_, cg_residual_, cg_update_, dot, maximum, minimum, norm, prod, vsum
from .sparse import (HPCSparseMatrix, HPCSparseMatrix_from_global, HPCSparseMatrix_local,
                     HPCSparseMatrix_local_device,
                     HostVectorPlan, VectorPlan, build_host_vector_plan, cache_sizes,
                     ExchangeTimeout, check_exchange_health,
                     clear_plan_cache, execute_plan, get_vector_plan, mul_, mul_dot_, split_column_map)
from .dense import (HPCMatrix, HPCMatrix_local, TransposedHPCMatrix, clear_dense_plan_cache, dense_matmat_t, dense_matvec,
                    dense_matvec_t, dense_sparse_matmat, dense_sparse_matmat_t)
from .spmm_plans import clear_spmm_cache, spmm, spmm_block_order_of, spmm_exchange_bytes, spmm_runs_fit_of
from .matmat import clear_matrix_plan_cache, get_matrix_plan, spgemm
from .krylov import CGInfo
from .cg import CGGraphPair, CGWorkspace, PCGWorkspace, cg, cg_fixed_iterations, cg_iterate, cg_setup
from .fsai import FSAI, fsai
from .amg import AMG, AMGLevel, AMGWorkspace, amg
from .ilu import ILU0, ilu0
from .bicgstab import BiCGStabWorkspace, bicgstab
from .gmres import GMRESWorkspace, gmres
from .lsqr import LSQRInfo, LSQRWorkspace, lsqr
from .minres import MinresWorkspace, minres
from .eigsh import EigshInfo, EigshWorkspace, eigsh
from .lobpcg import LobpcgInfo, LobpcgWorkspace, lobpcg
from .svds import SvdsInfo, SvdsWorkspace, svds
from .qr import lstsq, qr
from .convert import to_backend
from .transpose import (HostTransposeStructure, TransposedHPCSparseMatrix, TransposedHPCVector, TransposePlan,
                        DenseTransposeLists, HostSpmmTPlan, adjoint, clear_transpose_plan_cache, get_transpose_plan,
                        transpose)
from .addition import add_scaled_identity, sparse_add
from .indexing import SubmatrixPlan, diag, get_submatrix_plan
from .assemble import AssemblyPlan, assembly_plan, sparse_from_coo
from .select import SelectionPlan, VectorIndexPlan, index_plan, put_, select, selection_plan, take
from .rcm import RCMInfo, bandwidth, rcm
from .repartition import (RangePlan, SparseRepartitionPlan, clear_repartition_cache, exchange_ranges,
                          get_sparse_repartition_plan, get_vector_repartition_plan, repartition)

__all__ = [n for n in dir() if not n.startswith("_")] + ["_capi"]
