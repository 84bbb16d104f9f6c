/*
 * hpcla_rocm.h -- C ABI of libhpcla_rocm.so, the MI355X (gfx950) device library behind the
 * `DeviceROCm` backend of HPCLinearAlgebra.jl (sloisel/LinearAlgebraMPI.jl).
 *
 * Boundary.  The reference has no FFI for this path: its device work is Julia
 * KernelAbstractions kernels plus CPU-staged MPI.  The entry points below are what a
 * `ext/HPCLinearAlgebraROCmExt.jl` binds with `@ccall`, one per reference
 * function it replaces; each declaration cites that function (paths relative to the reference
 * repository root).  The pattern -- `ccall` returning an int status that the Julia wrapper checks --
 * is the one the reference already uses for cuDSS/NCCL (ext/HPCLinearAlgebraCUDAExt.jl:247-251,
 * 388-402).
 *
 * Conventions
 *  - plain pointers and sizes only; every data buffer is a DEVICE pointer owned by the caller
 *    (ROCArray / torch tensor / hipMalloc) unless the parameter name ends in `_host`;
 *  - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); all work is
 *    enqueued asynchronously, nothing synchronises the host unless documented;
 *  - return value: HPCLA_OK (0) or a negative status; hpcla_last_error() gives the text;
 *  - index arrays are int32 (`_i32`) or int64 (`_i64`, the reference default Ti=Int,
 *    src/backends.jl:348); `index_base` is 1 for arrays passed untouched from Julia
 *    (rowptr[1]==1, src/sparse.jl:2060) and 0 for C/Python callers;
 *  - handles (comm, halo plan) are library-owned, explicitly destroyed, never finalised with a
 *    collective (the reference's rule: ext/HPCLinearAlgebraCUDAExt.jl:9-10, 384-386);
 *  - not thread-safe per handle; re-entrant across handles.
 *
 * Arithmetic contract (fp64): every row sum is accumulated sequentially in stored order with a
 * separately rounded multiply and add (no FMA contraction), i.e. bit-identical to the reference
 * loop `acc += nzval[j] * x[colval[j]]` (src/sparse.jl:2055-2066) on IEEE hardware.
 */
#ifndef HPCLA_ROCM_H
#define HPCLA_ROCM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPCLA_VERSION 100 /* 0.1.0 */

/* status codes */
#define HPCLA_OK 0
#define HPCLA_ERR_INVALID -1     /* bad argument (null pointer, negative size, bad base/layout) */
#define HPCLA_ERR_HIP -2         /* a HIP runtime call failed */
#define HPCLA_ERR_RCCL -3        /* an RCCL call failed or librccl could not be loaded */
#define HPCLA_ERR_NO_DEVICE -4   /* no gfx950 device visible */
#define HPCLA_ERR_UNSUPPORTED -5 /* valid request this build does not implement */
#define HPCLA_ERR_ALLOC -6       /* device or host allocation failed */

/* dense layouts for SpMM operands: element (i,c) at ptr[i*ld + c] (ROW) or ptr[i + c*ld] (COL).
 * COL is Julia's Matrix (src/dense.jl:63); ROW is the device-native layout (one 128-byte line per
 * row at k=16). */
#define HPCLA_LAYOUT_ROW 0
#define HPCLA_LAYOUT_COL 1

typedef struct hpcla_comm hpcla_comm_t;           /* one RCCL communicator (or a serial stub) */
typedef struct hpcla_halo_plan hpcla_halo_plan_t; /* device half of a VectorPlan */

/* ---- library ------------------------------------------------------------------------------ */
int hpcla_version(void);
const char *hpcla_last_error(void);
/* Number of visible devices / select device for the calling thread (hipSetDevice).
 * Mirrors the rank->device assignment of ext/HPCLinearAlgebraCUDAExt.jl:611-613. */
int hpcla_device_count(int *count);
int hpcla_set_device(int device);
/* Device properties the host layer and bench report (CU count, arch name up to 63 chars). */
int hpcla_device_info(int device, int *num_cus, char *arch_name_host, int arch_name_len);

/* ---- SpMV:  replaces _spmv_kernel!/_spmv! (src/sparse.jl:2055-2084) ----------------------------
 * y[r] = sum_{j=rowptr[r]}^{rowptr[r+1]-1} nzval[j] * x[colval[j]],  r in [0,nrows).
 * `x` is the gathered vector x[col_indices] (length ncols_compressed), exactly the operand the
 * reference passes (`plan.gathered`, src/sparse.jl:2114-2119).  nnz = rowptr[nrows]-index_base is
 * passed by the caller (Julia: length(A.nzval)) so the launch needs no device->host read. */
int hpcla_spmv_csr_f64_i32(const int32_t *rowptr, const int32_t *colval, const double *nzval,
                           const double *x, double *y, int64_t nrows, int64_t nnz, int index_base,
                           void *stream);
int hpcla_spmv_csr_f64_i64(const int64_t *rowptr, const int64_t *colval, const double *nzval,
                           const double *x, double *y, int64_t nrows, int64_t nnz, int index_base,
                           void *stream);

/* Split-column SpMV used by the distributed path: a column index c < n_own reads x_own[c] (the
 * caller's HPCVector storage, x.v, untouched), c >= n_own reads x_ghost[c - n_own] (the halo
 * plan's receive segment).  This removes the reference's local gather loop
 * (src/vectors.jl:426-428, _gather_kernel! :174-177) from the hot path altogether.
 * `block_list` (device, int32, may be NULL) restricts the launch to the listed row blocks of
 * hpcla_spmv_rows_per_block() rows each -- the interior/boundary split.  colval is 0-based. */
int hpcla_spmv_split_f64_i32(const int32_t *rowptr, const int32_t *colval_split,
                             const double *nzval, const double *x_own, const double *x_ghost,
                             int64_t n_own, double *y, int64_t nrows, int64_t nnz, int index_base,
                             const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmv_split_f64_i64(const int64_t *rowptr, const int64_t *colval_split,
                             const double *nzval, const double *x_own, const double *x_ghost,
                             int64_t n_own, double *y, int64_t nrows, int64_t nnz, int index_base,
                             const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmv_rows_per_block(void);
/* The CSR SpMV kernel of every aligned launch (every entry point above and below; no reference counterpart -- the
 * reference has one work-item per row, src/sparse.jl:2055-2066) is the "row gather" (round 4): the block's A entries are
 * streamed into wave-private LDS unmultiplied and every lane walks its own row, so one gather instruction reads ONE x
 * stream for banded matrices (profiles/r04_spmv_2d_vs_3d_counters.txt).  The product-parking quad kernel of rounds 1-3 and
 * its switch (hpcla_set_spmv_kernel / hpcla_get_spmv_kernel, HPCLA_SPMV_KERNEL) were retired in round 6: it lost on every
 * measured matrix (profiles/r04_spmv_rowg.log).  Unaligned colval / nzval take a narrow fallback kernel, same bits. */
/* OPT-IN long rows (round 5; NOT the default, NOT bit-identical to the reference).  The default kernels sum every row
 * sequentially in stored order on one lane -- the reference's bits (acc += nzval[j] * x[colval[j]], src/sparse.jl:2059-2064)
 * and the reference's cliff: its _spmv_kernel! is one work-item per row too, so an "arrow" matrix (one dense row of n
 * entries) costs a whole sequential pass over that row.  This entry computes y = A*x with the rows listed in `long_rows`
 * (device array of 0-based row indices, exactly the rows that hold >= long_min >= 928 entries; at most 65535) summed in TREE
 * order -- 1024 contiguous pieces per row, wave shuffles inside a piece (north_star's "__shfl / segmented-scan row
 * reductions") -- and every other row exactly as hpcla_spmv_split_f64_* does, bit for bit.  A long row's result is within
 * 1e-12 * (|A||x|)_r of the sequential sum (tests: tests/test_gpu_parity.py::test_spmv_long_rows_opt_in).  x_ghost == NULL:
 * unsplit column space.  work: hpcla_spmv_longrows_work_bytes(n_long) bytes of device scratch.
 * A row of >= long_min entries that `long_rows` omits is not summed by anybody: its y is set to NaN (never left at a stale
 * value).  colval / nzval that are not 16- / 32-byte aligned take the default entry's fallback kernel (every row sequential). */
int64_t hpcla_spmv_longrows_work_bytes(int64_t n_long);
int hpcla_spmv_longrows_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                const double *x_own, const double *x_ghost, int64_t n_own, double *y,
                                int64_t nrows, int64_t nnz, int index_base, const int64_t *long_rows,
                                int64_t n_long, int64_t long_min, double *work, void *stream);
int hpcla_spmv_longrows_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                const double *x_own, const double *x_ghost, int64_t n_own, double *y,
                                int64_t nrows, int64_t nnz, int index_base, const int64_t *long_rows,
                                int64_t n_long, int64_t long_min, double *work, void *stream);
int hpcla_spmm_rows_per_block(void);
/* SpMM twins of the two block-order entries below (no reference counterpart: src/sparse.jl:2391-2413 is a column loop
 * over A*x in index order): the row blocks (hpcla_spmm_rows_per_block() rows each) of every SpMM launch over `rowptr`
 * -- a contiguous launch, or the POSITIONS of a block list -- are walked in XCD groups of `group` blocks.  Measured per
 * structure at plan time: the 5-point matrix loses with every group from 32 up, config 5's random pattern gains 2.6 %
 * at 64-256 (profiles/r03_spmm_xcd_group.log); the tuner times the plan's own launch (results go to the caller's C:
 * every launch writes the complete product) under natural / 16 / 64 / 256, keeps natural unless a group is >= 1 %
 * faster, and skips launches below 4096 row blocks, k < 2 and odd k on odd pitches.  B_ghost == NULL: the unsplit kernel. */
int hpcla_spmm_block_order_hint(const void *rowptr, int group);
int hpcla_spmm_tune_block_order_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                        const double *B_own, int64_t ldb_own, const double *B_ghost, int64_t ldb_ghost,
                                        int64_t n_own, double *C, int64_t ldc, int64_t nrows, int64_t nnz, int k,
                                        int index_base, const int32_t *block_list, int64_t n_blocks, void *stream,
                                        int *chosen_group);
int hpcla_spmm_tune_block_order_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                        const double *B_own, int64_t ldb_own, const double *B_ghost, int64_t ldb_ghost,
                                        int64_t n_own, double *C, int64_t ldc, int64_t nrows, int64_t nnz, int k,
                                        int index_base, const int32_t *block_list, int64_t n_blocks, void *stream,
                                        int *chosen_group);

/* Optional plan-time performance hint (no reference counterpart: the reference launches one work-item per row in
 * index order, src/sparse.jl:2055-2066, 2081-2082): SpMV launches over the matrix whose `rowptr` device pointer is
 * given walk their contiguous runs of row blocks in an XCD-grouped order -- groups of `group` consecutive row blocks
 * per XCD, groups dealt round-robin -- so that row blocks whose columns overlap share one of the 8 L2s (config 4's
 * 512 x 512 planes: neighbours two blocks apart; -2 to -5 % per SpMV on every stencil matrix measured).  `group` = 0 or 1 removes the hint (natural order);
 * otherwise a power of two <= 1024.  Results are bit-identical in every order (each row is still one sequential sum);
 * launches restricted to a block LIST keep the list's order.  Keyed by the pointer: remove the hint before the
 * array is freed (a stale entry can only cost performance).  Thread-safe. */
int hpcla_spmv_block_order_hint(const void *rowptr, int group);

/* Plan-time choice of that order BY MEASUREMENT (run once per structure, next to the VectorPlan build of
 * src/sparse.jl:1875-1984, never inside a timed or captured region: it synchronises): times the split-column SpMV of
 * this matrix -- the arguments of hpcla_spmv_split_f64_*, results discarded into `y_scratch` (nrows doubles) -- under the
 * natural order and groups of 8 / 32 / 64 row blocks, interleaved over one warm-up round of two launches and five
 * counted rounds of eight launches each (168 launches, with the alternating sweep below active), keeps the winner by
 * hpcla_block_order_decide registered for `rowptr` and returns it in *chosen_group (1 = natural).  Matrices below 4096
 * row blocks keep the natural order unmeasured. */
int hpcla_spmv_tune_block_order_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                        const double *x_own, const double *x_ghost, int64_t n_own, double *y_scratch,
                                        int64_t nrows, int64_t nnz, int index_base, void *stream, int *chosen_group);
int hpcla_spmv_tune_block_order_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                        const double *x_own, const double *x_ghost, int64_t n_own, double *y_scratch,
                                        int64_t nrows, int64_t nnz, int index_base, void *stream, int *chosen_group);

/* The tuner's decision rule alone (host code, no device work).  ms[c * n_rounds + r] is the time of candidate c in counted
 * round r; candidate 0 is the natural order.  A grouped candidate is kept only if it beat the natural order in EVERY
 * round (compared pair by pair within the round) and the median of its ratios to the natural order is <= 0.99; of those
 * the smallest median wins, the first on a tie; otherwise *chosen_index = 0.  Null pointers, n_cand < 1, n_rounds
 * outside 1 ... 64 and times that are not positive and finite are HPCLA_ERR_INVALID. */
int hpcla_block_order_decide(const float *ms, int n_cand, int n_rounds, int *chosen_index);

/* Sweep direction of repeated products (no reference counterpart).  A plain SpMV launch over a contiguous run of row
 * blocks -- every entry above without a block list, every index form, with or without the dot epilogue -- that repeats
 * the calling thread's last such launch (same rowptr, nzval, nrows and run) walks the run in the opposite direction, so
 * that it starts on the lines the last launch left in the Infinity Cache and the L2s; every row block stays on its XCD.
 * Anything else starts forwards.  Results are bit-identical in both directions (each row is still one sequential sum,
 * dot partials stay indexed by row block).  Listed launches and the fused distributed launch always go forwards.
 * mode: 0 every launch forwards, 1 alternate, -1 back to the default (alternate); process-wide.  The library reads no
 * environment variable for it: the Python host layer applies HPCLA_SPMV_SWEEP=forward|alternate through this call when
 * it loads the library.  hpcla_spmv_last_sweep: *reversed = 1 if the calling thread's last plain contiguous launch went
 * downwards, else 0 (also before any launch). */
int hpcla_set_spmv_sweep(int mode);
int hpcla_spmv_last_sweep(int *reversed);

/* Plan-time helpers (run once per (A, x.partition), cached with the VectorPlan like
 * _vector_plan_cache, src/HPCLinearAlgebra.jl:133).
 * remap: out[j] = map[in[j] - index_base]   (compressed column -> split column; out is 0-based)
 * classify: flags[b] = 1 if row block b (rows_per_block rows: hpcla_spmv_rows_per_block() or
 *           hpcla_spmm_rows_per_block()) references any column >= n_own, else 0. */
int hpcla_remap_i32(const int32_t *in, const int32_t *map, int32_t *out, int64_t n, int index_base,
                    void *stream);
int hpcla_remap_i64(const int64_t *in, const int64_t *map, int64_t *out, int64_t n, int index_base,
                    void *stream);
/* Plan-time NARROWING of an Int64 structure.  The reference's default index type is Ti = Int (src/backends.jl:348,
 * 369: backend_cpu_serial / backend_cpu_mpi default to Int), so a caller who follows the defaults hands over Int64
 * rowptr / colval although every BASELINE configuration fits Int32 per GPU.  Indices are never results: when
 * nnz + index_base and n_own + n_ghost + index_base fit Int32, the plan keeps Int32 copies (remap_i64_to_i32: the
 * split colval straight from the Int64 compressed colval through an Int32 map; narrow_i64_to_i32: rowptr) and every
 * launch over that plan takes the _i32 kernels -- 12 instead of 16 index+value bytes per stored entry, same bits.
 * narrow: if `overflow_dev` is not NULL, *overflow_dev |= 1 when a value does not fit (the caller zeroes it). */
int hpcla_remap_i64_to_i32(const int64_t *in, const int32_t *map, int32_t *out, int64_t n, int index_base,
                           void *stream);
int hpcla_narrow_i64_to_i32(const int64_t *in, int32_t *out, int64_t n, uint32_t *overflow_dev, void *stream);
int hpcla_classify_blocks_i32(const int32_t *rowptr, const int32_t *colval_split, int64_t nrows,
                              int index_base, int64_t n_own, int rows_per_block, int32_t *flags,
                              void *stream);
int hpcla_classify_blocks_i64(const int64_t *rowptr, const int64_t *colval_split, int64_t nrows,
                              int index_base, int64_t n_own, int rows_per_block, int32_t *flags,
                              void *stream);

/* ---- device-side construction: replaces the host sort + per-nonzero binary search of
 * HPCSparseMatrix_local (col_indices = unique!(sort(rowval)), compress_AT; src/sparse.jl:501-509,
 * 137-144) by a presence bitmap + exclusive scan + emit pass over a column window.
 * colidx_global: this rank's nonzeros' GLOBAL 0-based columns (device int64); every id must lie in
 * [col_lo, col_lo+window).  Outputs: colval_out (local index + index_base per nonzero),
 * col_indices_out (device int64, capacity `window`; first *ncols_compressed_host entries valid,
 * ascending).  `work`: hpcla_colspace_work_bytes(window) device bytes.  Synchronises the stream. */
int64_t hpcla_colspace_work_bytes(int64_t window);
/* 256-bit order-sensitive digest of a device index array (the local pass of compute_structural_hash,
 * src/sparse.jl:97-121, without a D2H copy of colval): out_host[k] = sum_i mix(a[i]*P1 + (i+1)*P2 + S_k)
 * mod 2^64, k = 0..3.  Memoization keys only -- compared for equality, like the reference's Blake3
 * digests.  Synchronises the stream. */
int hpcla_digest_i32(const int32_t *a, int64_t n, uint64_t *out_host /* 4 words */, void *stream);
int hpcla_digest_i64(const int64_t *a, int64_t n, uint64_t *out_host /* 4 words */, void *stream);
int hpcla_compress_columns_i32(const int64_t *colidx_global, int64_t nnz, int64_t col_lo, int64_t window,
                               int32_t *colval_out, int index_base, int64_t *col_indices_out,
                               int64_t *ncols_compressed_host, void *work, void *stream);
int hpcla_compress_columns_i64(const int64_t *colidx_global, int64_t nnz, int64_t col_lo, int64_t window,
                               int64_t *colval_out, int index_base, int64_t *col_indices_out,
                               int64_t *ncols_compressed_host, void *work, void *stream);
/* On-device generator of the BASELINE stencil workload (create_2d_laplacian,
 * test/test_factorization.jl:60-102): rows [row_start,row_end) of the nx*ny 5-point Laplacian as
 * CSR with GLOBAL 0-based columns (rowptr_out: row_end-row_start+1 int64, 0-based). */
int64_t hpcla_poisson2d_nnz(int64_t nx, int64_t ny, int64_t row_start, int64_t row_end);
int hpcla_gen_poisson2d(int64_t nx, int64_t ny, int64_t row_start, int64_t row_end, int64_t *rowptr_out,
                        int64_t *colidx_out, double *vals_out, void *stream);
/* the 7-point analogue of BASELINE configs[3] (idx = (k*ny + j)*nx + i, diagonal 6) */
int64_t hpcla_poisson3d_nnz(int64_t nx, int64_t ny, int64_t nz, int64_t row_start, int64_t row_end);
int hpcla_gen_poisson3d(int64_t nx, int64_t ny, int64_t nz, int64_t row_start, int64_t row_end,
                        int64_t *rowptr_out, int64_t *colidx_out, double *vals_out, void *stream);

/* ---- range indexing of a sparse matrix: A[r0:r1, c0:c1] and A[:, k] (csrc/submatrix.hip) ------------------------
 * Replaces the host walk over `_get_csc(A)` of Base.getindex(A::HPCSparseMatrix, ::UnitRange, ::UnitRange)
 * (src/indexing.jl:691-840: count and collect :775-794, per-row sort :796-805, recompression :807-819) and of
 * Base.getindex(A, :, k) (src/indexing.jl:872-914, the scan :891-908).  No communication, as in the reference
 * (_compute_subpartition, src/indexing.jl:38-62, stays on the host).
 *
 * Relies on the struct's invariants: col_indices sorted, so a global column window is ONE window [j0, j1) of compressed
 * local columns; columns ascending within a row (src/sparse.jl:288-295), so a row keeps ONE contiguous run of its entries.
 * The windows are 0-based and half-open whatever `index_base` is: local rows [r0, r1) of [0, nrows], local compressed
 * columns [j0, j1).  rowptr / colval (in and out) carry `index_base`; src_start is always a 0-based entry position.
 * Values are moved by size: elem_bytes = 8 (Float64) or 4 (Float32); every bit of a kept entry survives.
 *
 * structure: src_start_out[i] / rowptr_out[i] for the r1 - r0 selected rows (rowptr_out has r1 - r0 + 1 entries),
 *   col_indices_out (device int64, capacity j1 - j0): the kept columns that occur, ascending, as
 *   col_indices_src[j] - col_shift (col_indices_src: the source's global column ids on the device; NULL: the local j).
 *   Returns the new nnz and the new compressed column count to the host: synchronises the stream once, like
 *   hpcla_compress_columns_*.  `work`: hpcla_submatrix_work_bytes(r1 - r0, j1 - j0) device bytes; it holds the column
 *   look-up table that `fill` reads, so it must live until the fill has run.
 * fill: colval_out / nzval_out (nnz_out entries each) from the structure pass's outputs.  No synchronisation.
 * values: nzval_out alone, from the src_start and rowptr_out of an earlier extraction (the source may be any matrix of
 *   the same structure).  No synchronisation.
 * hpcla_submatrix_scan_chunk: elements per workgroup of the scan behind rowptr_out and col_indices_out (tests cross it). */
int64_t hpcla_submatrix_work_bytes(int64_t nsel, int64_t width);
int64_t hpcla_submatrix_scan_chunk(void);
int hpcla_submatrix_structure_i32(const int32_t *rowptr, const int32_t *colval, int64_t nrows, int64_t nnz, int64_t r0,
                                  int64_t r1, int64_t j0, int64_t j1, int index_base, const int64_t *col_indices_src,
                                  int64_t col_shift, int64_t *src_start_out, int32_t *rowptr_out, int64_t *col_indices_out,
                                  int64_t *nnz_out_host, int64_t *ncols_out_host, void *work, void *stream);
int hpcla_submatrix_structure_i64(const int64_t *rowptr, const int64_t *colval, int64_t nrows, int64_t nnz, int64_t r0,
                                  int64_t r1, int64_t j0, int64_t j1, int index_base, const int64_t *col_indices_src,
                                  int64_t col_shift, int64_t *src_start_out, int64_t *rowptr_out, int64_t *col_indices_out,
                                  int64_t *nnz_out_host, int64_t *ncols_out_host, void *work, void *stream);
int hpcla_submatrix_fill_i32(int elem_bytes, const int32_t *colval, const void *nzval, int64_t nnz_src,
                             const int64_t *src_start, const int32_t *rowptr_out, int64_t nsel, int64_t nnz_out, int64_t j0,
                             int64_t j1, int index_base, const void *work, int32_t *colval_out, void *nzval_out, void *stream);
int hpcla_submatrix_fill_i64(int elem_bytes, const int64_t *colval, const void *nzval, int64_t nnz_src,
                             const int64_t *src_start, const int64_t *rowptr_out, int64_t nsel, int64_t nnz_out, int64_t j0,
                             int64_t j1, int index_base, const void *work, int64_t *colval_out, void *nzval_out, void *stream);
int hpcla_submatrix_values_i32(int elem_bytes, const void *nzval, int64_t nnz_src, const int64_t *src_start,
                               const int32_t *rowptr_out, int64_t nsel, int64_t nnz_out, int index_base, void *nzval_out,
                               void *stream);
int hpcla_submatrix_values_i64(int elem_bytes, const void *nzval, int64_t nnz_src, const int64_t *src_start,
                               const int64_t *rowptr_out, int64_t nsel, int64_t nnz_out, int index_base, void *nzval_out,
                               void *stream);
/* A[:, k] (src/indexing.jl:891-908): out[i] = the stored value of local compressed column jk (0-based) in local row i,
 * +0.0 where the row stores none.  The caller handles a k that is not among col_indices (all zeros, no kernel). */
int hpcla_sparse_column_i32(int elem_bytes, const int32_t *rowptr, const int32_t *colval, const void *nzval, int64_t nrows,
                            int64_t nnz, int64_t jk, int index_base, void *out, void *stream);
int hpcla_sparse_column_i64(int elem_bytes, const int64_t *rowptr, const int64_t *colval, const void *nzval, int64_t nrows,
                            int64_t nnz, int64_t jk, int index_base, void *out, void *stream);
/* diag(A) (LinearAlgebra.diag on a square HPCSparseMatrix): out[i] = the stored value of (i, row_start + i) bit for bit,
 * +0.0 where the row stores none; i is the local row, row_start this rank's first global row (0-based), col_indices
 * (n_col_indices sorted global column ids, 0-based, device memory) the matrix's compressed-column table.  One lane per
 * row, the look-up of hpcla_sparse_column_* with a per-row key.  reciprocal != 0 writes 1 / value instead (the Jacobi
 * preconditioner of hp.cg; a missing entry gives +inf).  Float64 values. */
int hpcla_sparse_diag_f64_i32(const int32_t *rowptr, const int32_t *colval, const double *nzval, int64_t nrows, int64_t nnz,
                              int index_base, const int64_t *col_indices, int64_t n_col_indices, int64_t row_start,
                              int reciprocal, double *out, void *stream);
int hpcla_sparse_diag_f64_i64(const int64_t *rowptr, const int64_t *colval, const double *nzval, int64_t nrows, int64_t nnz,
                              int index_base, const int64_t *col_indices, int64_t n_col_indices, int64_t row_start,
                              int reciprocal, double *out, void *stream);

/* ---- index-set selection: A[rows, cols] for index lists, v[idx], v[idx] = src (csrc/select.hip) -------------------
 * Replaces Base.getindex(A::HPCSparseMatrix, row_idx::HPCVector{Int}, col_idx::HPCVector{Int}) (src/indexing.jl:1654-1815:
 * the Dict from column to position :1675-1678, the walk of every selected row through it, extract_sparse_row :1743-1765),
 * Base.getindex(v, idx) (:1339-1460) and Base.setindex!(v, src, idx) (:1871-1985).  The reference returns a DENSE
 * HPCMatrix (:1640-1644); these entries build the CSR of a sparse result.  The caller gathers the ranks' column lists
 * (:1662, 1821-1844), sorts the list stably with its positions (any sort) and refuses duplicates; the library does the rest.
 *
 * A kept entry goes to rowptr'[r] + (the number of kept entries of its row with a smaller new column): new columns are
 * distinct within a row, so the ranks are unique, columns ascend within every output row and nothing but integers is
 * compared.  Values are moved by size (elem_bytes 8 or 4): every bit survives.  `rows`, `sorted_pos` and `src_out` are
 * 0-based positions whatever `index_base` is; rowptr / colval (in and out), col_indices_src, sorted_cols and
 * col_indices_out carry `index_base`.
 *
 * structure: `rows` (nsel local rows in output order, repeats allowed; NULL: rows 0 .. nsel - 1), `sorted_cols` (nsorted
 *   global column ids, ascending, distinct) with `sorted_pos` (the position of each in the caller's list: the new global
 *   column, in [0, width)); nsorted = -1: all columns in order (new column = old column, width = the matrix's).  Writes
 *   rowptr_out (nsel + 1) and col_indices_out (capacity min(width, ncomp): the new columns that occur, ascending); returns
 *   the new nnz, the new compressed column count and the longest kept row to the host: synchronises the stream once.
 *   Where the new nnz (plus index_base) does not fit the index type, rowptr_out has wrapped: the three host values are
 *   still returned, the status is HPCLA_ERR_UNSUPPORTED, and rowptr_out must not be used.
 *   `work`: hpcla_select_work_bytes(nsel, ncomp, width) device bytes; it starts with the table from A's compressed column
 *   to the result's that `fill` reads, so it must live until the fill has run.
 * fill: colval_out / nzval_out / src_out (nnz_out entries each; src_out[p] = the position in the source's nzval of output
 *   entry p).  Three forms by kept row length n: n <= hpcla_select_short_cap() (lane groups), n <= hpcla_select_tile() (a
 *   workgroup per row, the row in LDS), longer (a workgroup per row, every tile ranked against the whole row: quadratic,
 *   the slow case).  max_row: the longest kept row as `structure` returned it, or -1 when unknown; the two long forms are
 *   launched only when it asks for them.  No synchronisation.
 * values of another matrix of the same structure: out[p] = nzval2[src_out[p]]: hpcla_gather_f64_i64 for 8-byte elements,
 *   hpcla_gather_b32_i64 for 4-byte ones (x holds nx items; a position outside reads as 0).
 * take: out[i] = p < n_own ? v[p] : ghost[p - n_own] for p = pos[i] - index_base (outside both: +0.0).
 * put:  v[p] = src[i] for p = pos[i] - index_base in [0, n_own); positions must be distinct.  _i32 / _i64: the width of pos. */
int64_t hpcla_select_short_cap(void);
int64_t hpcla_select_tile(void);
int64_t hpcla_select_work_bytes(int64_t nsel, int64_t ncomp, int64_t width);
int hpcla_select_structure_i32(const int32_t *rowptr, const int32_t *colval, int64_t nrows, int64_t nnz,
                               const int64_t *col_indices_src, int64_t ncomp, const int64_t *rows, int64_t nsel,
                               const int64_t *sorted_cols, const int64_t *sorted_pos, int64_t nsorted, int64_t width,
                               int index_base, int32_t *rowptr_out, int64_t *col_indices_out, int64_t *nnz_out_host,
                               int64_t *ncols_out_host, int64_t *max_row_host, void *work, void *stream);
int hpcla_select_structure_i64(const int64_t *rowptr, const int64_t *colval, int64_t nrows, int64_t nnz,
                               const int64_t *col_indices_src, int64_t ncomp, const int64_t *rows, int64_t nsel,
                               const int64_t *sorted_cols, const int64_t *sorted_pos, int64_t nsorted, int64_t width,
                               int index_base, int64_t *rowptr_out, int64_t *col_indices_out, int64_t *nnz_out_host,
                               int64_t *ncols_out_host, int64_t *max_row_host, void *work, void *stream);
int hpcla_select_fill_i32(int elem_bytes, const int32_t *rowptr, const int32_t *colval, const void *nzval, int64_t nrows,
                          int64_t nnz, int64_t ncomp, const int64_t *rows, int64_t nsel, const int32_t *rowptr_out,
                          int64_t nnz_out, int64_t max_row, int index_base, const void *work, int32_t *colval_out,
                          void *nzval_out, int64_t *src_out, void *stream);
int hpcla_select_fill_i64(int elem_bytes, const int64_t *rowptr, const int64_t *colval, const void *nzval, int64_t nrows,
                          int64_t nnz, int64_t ncomp, const int64_t *rows, int64_t nsel, const int64_t *rowptr_out,
                          int64_t nnz_out, int64_t max_row, int index_base, const void *work, int64_t *colval_out,
                          void *nzval_out, int64_t *src_out, void *stream);
int hpcla_gather_b32_i64(const void *x, const int64_t *src, void *out, int64_t n, int64_t nx, int index_base, void *stream);
int hpcla_select_take_f64_i32(const double *v, int64_t n_own, const double *ghost, int64_t n_ghost, const int32_t *pos,
                              int64_t n, int index_base, double *out, void *stream);
int hpcla_select_take_f64_i64(const double *v, int64_t n_own, const double *ghost, int64_t n_ghost, const int64_t *pos,
                              int64_t n, int index_base, double *out, void *stream);
int hpcla_select_put_f64_i32(double *v, int64_t n_own, const int32_t *pos, const double *src, int64_t n, int index_base,
                             void *stream);
int hpcla_select_put_f64_i64(double *v, int64_t n_own, const int64_t *pos, const double *src, int64_t n, int index_base,
                             void *stream);

/* ---- reverse Cuthill-McKee ordering of a rank's owned block, and the bandwidth (hp.rcm, hp.bandwidth, csrc/rcm.hip) -----
 * No reference counterpart: the reference never reorders.  Rows and columns of A are partitioned alike; a stored entry whose
 * global column (col_indices_dev[colval - index_base] - index_base) lies in [row_start, row_start + nrows) names the local
 * row column - row_start, every other entry and the diagonal are dropped.  Only structure is read.  nrows < 2^31 - 1 and fewer
 * than 2^31 graph entries (the caller checks the latter from info_dev).
 *   rcm_work_bytes      device bytes of `work` for the count's scan.
 *   rcm_graph_count / _fill   g_rowptr_dev (nrows + 1, int64, 0-based), info_dev[0] = the graph's entries; then g_cols_dev
 *                       (int32 local columns, stored order kept).
 *   rcm_degrees         deg_dev[i] = the entries of row i of a graph; distinct != 0: the entries that no earlier entry of the
 *                       row repeats (quadratic in the row), for a graph from hpcla_amg_symmetrise_fill, which lists an edge
 *                       stored both ways twice.
 *   rcm_init            by_degree_dev: the vertices sorted by (deg, index), the caller's stable sort.  rank_dev = its inverse,
 *                       parent_dev = 2^31 - 1 (unvisited); the z vertices without a neighbour take order_dev[0 .. z) in index
 *                       order and parent = their number; info_dev[0] = z.
 * The walk numbers vertices into order_dev; order_dev[lo .. hi) is the current level, hi the next free number.  parent_dev is
 * touched by agent-scope atomics only: an atomic min with the number of the level vertex claims, the lane that finds 2^31 - 1
 * appends the neighbour to the candidates.  New vertices are numbered in ascending (parent << 32) | rank.
 *   rcm_narrow          ONE workgroup walks levels while the frontier has at most hpcla_rcm_frontier_cap() vertices and its row
 *                       lengths sum to at most hpcla_rcm_candidate_cap() (tested before parent is touched); frontier, keys and
 *                       the bitonic sort live in LDS; a component that ends is followed by the first unvisited vertex of
 *                       by_degree at or after `cursor`.  first_dev != NULL: lo = hi = cursor = first_dev[0] (rcm_init's z).
 *                       record_dev (6 words): lo, hi, cursor, status (0: all nrows numbered, 1: the level [lo, hi) exceeds a
 *                       cap and is untouched, 2: internal error), the levels walked and the components started in this call
 *                       (a start is a level).  Waits on nothing but its own barrier.
 *   rcm_expand          one level of any size: claims the neighbours of order_dev[lo .. hi), a lane group per vertex and chunk
 *                       of 256 neighbours (longest_row: the longest row of the graph); cand_dev (nrows words) takes the claimed
 *                       vertices in no defined order, count_dev[0] (reset here) their number: one atomic add per wave.
 *   rcm_keys            keys_dev[i] = (parent << 32) | rank of cand_dev[i], in a launch after the expand.
 *   rcm_number          order_dev[cnt + i] = by_degree_dev[keys_dev[i] & 0xffffffff] for the SORTED keys (the caller's sort).
 *   rcm_finish          p_dev[i] = order_dev[nrows - 1 - i] + row_start (int64), inv_dev[order_dev[nrows - 1 - i]] = i.
 *   rcm_graph_bandwidth out_dev[0] = max |inv[i] - inv[c]| over the graph's entries (inv_dev == NULL: |i - c|).
 *   bandwidth           out_dev[0] = max |row_start + i - global column| over every stored entry of rows 0 .. nrows - 1.
 * Both maxima: an integer maximum per workgroup, then one atomic max.  Integer atomics only; all only enqueue; every result
 * is fixed by the inputs. */
int64_t hpcla_rcm_frontier_cap(void);
int64_t hpcla_rcm_candidate_cap(void);
int64_t hpcla_rcm_work_bytes(int64_t nrows);
int hpcla_rcm_graph_count_i32(const int32_t *rowptr, const int32_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                              int64_t row_start, int index_base, int64_t *g_rowptr_dev, int64_t *info_dev, void *work,
                              void *stream);
int hpcla_rcm_graph_count_i64(const int64_t *rowptr, const int64_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                              int64_t row_start, int index_base, int64_t *g_rowptr_dev, int64_t *info_dev, void *work,
                              void *stream);
int hpcla_rcm_graph_fill_i32(const int32_t *rowptr, const int32_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                             int64_t row_start, int index_base, const int64_t *g_rowptr_dev, int32_t *g_cols_dev, void *stream);
int hpcla_rcm_graph_fill_i64(const int64_t *rowptr, const int64_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                             int64_t row_start, int index_base, const int64_t *g_rowptr_dev, int32_t *g_cols_dev, void *stream);
int hpcla_rcm_degrees(const int64_t *g_rowptr_dev, const int32_t *g_cols_dev, int64_t nrows, int distinct, int32_t *deg_dev,
                      void *stream);
int hpcla_rcm_init(const int32_t *deg_dev, const int32_t *by_degree_dev, int64_t nrows, int32_t *rank_dev, int32_t *parent_dev,
                   int32_t *order_dev, int64_t *info_dev, void *stream);
int hpcla_rcm_narrow(const int64_t *g_rowptr_dev, const int32_t *g_cols_dev, const int32_t *by_degree_dev, const int32_t *rank_dev,
                     int64_t nrows, int64_t lo, int64_t hi, int64_t cursor, const int64_t *first_dev, int32_t *parent_dev,
                     int32_t *order_dev, int64_t *record_dev, void *stream);
int hpcla_rcm_expand(const int64_t *g_rowptr_dev, const int32_t *g_cols_dev, int64_t nrows, const int32_t *order_dev, int64_t lo,
                     int64_t hi, int64_t longest_row, int32_t *parent_dev, int32_t *cand_dev, int64_t *count_dev, void *stream);
int hpcla_rcm_keys(const int32_t *cand_dev, int64_t ncand, int64_t nrows, int32_t *parent_dev, const int32_t *rank_dev,
                   int64_t *keys_dev, void *stream);
int hpcla_rcm_number(const int64_t *keys_dev, int64_t ncand, int64_t nrows, const int32_t *by_degree_dev, int64_t cnt,
                     int32_t *order_dev, void *stream);
int hpcla_rcm_finish(const int32_t *order_dev, int64_t nrows, int64_t row_start, int64_t *p_dev, int32_t *inv_dev, void *stream);
int hpcla_rcm_graph_bandwidth(const int64_t *g_rowptr_dev, const int32_t *g_cols_dev, int64_t nrows, const int32_t *inv_dev,
                              int64_t *out_dev, void *stream);
int hpcla_bandwidth_i32(const int32_t *rowptr, const int32_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                        int64_t row_start, int index_base, int64_t *out_dev, void *stream);
int hpcla_bandwidth_i64(const int64_t *rowptr, const int64_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                        int64_t row_start, int index_base, int64_t *out_dev, void *stream);

/* ---- COO assembly with a reusable structure: sparse(I, J, V, m, n) on the device (csrc/assemble.hip) --------------
 * Replaces the host idiom sparse(I, J, V, m, n) + HPCSparseMatrix(A, backend) (src/sparse.jl:398-413) of a loop that
 * produces new values V on the same (I, J) at every step.  The structure is an inverted index: the caller sorts the keys
 * (row - row_lo) * ncols + col STABLY (any sort; the library's Python layer uses torch.sort) and keeps the permutation
 * `perm`; `seg_ptr` cuts the sorted list where the key changes; output entry e is the sum of the values at the positions
 * perm[seg_ptr[e]] ... perm[seg_ptr[e + 1] - 1], which ascend.  No float atomics anywhere.
 *
 * Sum order (it fixes the bits; CH = hpcla_assemble_chunk()).  A segment of L <= CH contributions: s = v[p1];
 * s = s + v[p2]; ... left to right, started from the first value and not from 0.0, so a lone -0.0 stays -0.0.  L > CH:
 * consecutive chunks of CH contributions, each summed by that rule, and the partial sums added left to right in chunk
 * order.  Only adds occur: the result does not depend on contraction, and two calls give the same bits.  A segment
 * without contributions (the vector form) stores +0.0.
 *
 * Positions (seg_ptr, perm) are always 0-based; rows / cols in and rowptr / column ids out carry `index_base`.  The
 * _i32 / _i64 suffix is the width of seg_ptr and perm (int32 needs the list length <= 2^31 - 1), except for row_starts,
 * where it is the width of the output.
 *
 * keys: key_out[i] = (rows[i] - row_lo) * ncols + cols[i] for a triplet of this rank's rows [row_lo, row_hi); cols NULL
 *   with ncols 1 is the vector form.  counts_dev (device, 4 words, set here): [0] triplets with a row outside
 *   [0, nrows_global) or a column outside [0, ncols), [1] the first such position or -1, [2] triplets inside the matrix
 *   but outside this rank's rows, [3] the first such position or -1.  A refused triplet gets the key INT64_MAX.  Needs
 *   (row_hi - row_lo) * ncols < 2^63.  No synchronisation.
 * segments: seg_ptr_out (capacity n + 1) and ukey_out (capacity n; the distinct keys, ascending) from the sorted keys;
 *   the number of segments returns to the host: synchronises the stream once, like hpcla_compress_columns_*.  `work`:
 *   hpcla_assemble_work_bytes(n) device bytes.  Elements per workgroup of the scan: hpcla_submatrix_scan_chunk().
 * row_starts: out[r] = index_base + the first position of keys_sorted whose key is >= r * ncols, for r in [0, nrows]
 *   (nrows + 1 words).  Over the distinct keys this is rowptr; over the sorted keys of the vector form (ncols 1) it is
 *   seg_ptr, with an empty segment for every index nothing contributes to.  No synchronisation.
 * columns: colidx_out[u] = ukey[u] mod ncols + index_base.  No synchronisation.
 * values: out[e] for e in [0, nseg).  The rank's value list is [vals (n_own) | ghost (n_ghost)]: a position p of perm
 *   reads vals[p] if p < n_own, else ghost[p - n_own]; a position outside both reads as +0.0.  n_in: the length of perm.
 *   A workgroup owns hpcla_assemble_run() consecutive output entries and walks its span of the list in passes of
 *   hpcla_assemble_pass() contributions (tests cross both).  max_len: an upper bound of the segment lengths, or -1 when
 *   unknown; when it exceeds CH (or is -1) a first launch sums the chunks of the long segments on separate waves into
 *   `work` (hpcla_assemble_values_work_bytes(n_in) device bytes, else it may be NULL), and the long entries add their
 *   partial sums in chunk order.  A max_len below the true maximum leaves +0.0 in the longer entries.  Plain stores, no
 *   read-back, no synchronisation. */
int64_t hpcla_assemble_chunk(void);
int64_t hpcla_assemble_run(void);
int64_t hpcla_assemble_pass(void);
int64_t hpcla_assemble_work_bytes(int64_t n);
int64_t hpcla_assemble_values_work_bytes(int64_t n_in);
int hpcla_assemble_keys(const int64_t *rows, const int64_t *cols, int64_t n, int64_t row_lo, int64_t row_hi,
                        int64_t nrows_global, int64_t ncols, int index_base, int64_t *key_out, int64_t *counts_dev,
                        void *stream);
int hpcla_assemble_segments_i32(const int64_t *keys_sorted, int64_t n, int32_t *seg_ptr_out, int64_t *ukey_out,
                                int64_t *nnz_out_host, void *work, void *stream);
int hpcla_assemble_segments_i64(const int64_t *keys_sorted, int64_t n, int64_t *seg_ptr_out, int64_t *ukey_out,
                                int64_t *nnz_out_host, void *work, void *stream);
int hpcla_assemble_row_starts_i32(const int64_t *keys_sorted, int64_t n, int64_t nrows, int64_t ncols, int index_base,
                                  int32_t *out, void *stream);
int hpcla_assemble_row_starts_i64(const int64_t *keys_sorted, int64_t n, int64_t nrows, int64_t ncols, int index_base,
                                  int64_t *out, void *stream);
int hpcla_assemble_columns(const int64_t *ukey, int64_t nnz, int64_t ncols, int index_base, int64_t *colidx_out,
                           void *stream);
int hpcla_assemble_values_f64_i32(const int32_t *seg_ptr, const int32_t *perm, int64_t nseg, int64_t n_in,
                                  const double *vals, int64_t n_own, const double *ghost, int64_t n_ghost, int64_t max_len,
                                  double *out, void *work, void *stream);
int hpcla_assemble_values_f64_i64(const int64_t *seg_ptr, const int64_t *perm, int64_t nseg, int64_t n_in,
                                  const double *vals, int64_t n_own, const double *ghost, int64_t n_ghost, int64_t max_len,
                                  double *out, void *work, void *stream);

/* ---- SpGEMM local product (sparse x sparse): replaces the CPU SparseArrays multiply inside
 * Base.:*(A::HPCSparseMatrix, B::HPCSparseMatrix) (`CT = plan.AT * A_csc`, src/sparse.jl:991-1059).
 * G = the rows of B named by A.col_indices, gathered by the MatrixPlan (src/sparse.jl:554-978), as
 * CSR with int64 rowptr and GLOBAL int64 columns; A's colval indexes G's rows.  Each C(i,j) is the sum
 * over k ascending of separately rounded G(k,j)*A(i,k), first product assigned -- the reference order.
 *  ub:       ub_out[i] = sum of the lengths of the G rows that row i references
 *  numeric:  rows `row_list` (all with ub <= hpcla_spgemm_bin_cap(bin); bins 0,1,... until the cap is
 *            -1; G's column ids must be < 2^58) -> sorted (col,val) runs at c_*_tmp[ub_prefix[i] ...]
 *            and their lengths cnt[i]
 *  compact:  c_rowptr (exclusive scan of cnt) -> final CSR arrays */
int64_t hpcla_spgemm_bin_cap(int bin);
int hpcla_spgemm_ub_i32(const int32_t *a_rowptr, const int32_t *a_col, int64_t nrows, int index_base,
                        const int64_t *g_rowptr, int64_t *ub_out, void *stream);
int hpcla_spgemm_ub_i64(const int64_t *a_rowptr, const int64_t *a_col, int64_t nrows, int index_base,
                        const int64_t *g_rowptr, int64_t *ub_out, void *stream);
int hpcla_spgemm_numeric_i32(int bin, const int32_t *a_rowptr, const int32_t *a_col, const double *a_val,
                             int index_base, const int64_t *g_rowptr, const int64_t *g_col,
                             const double *g_val, const int32_t *row_list, int64_t n_list,
                             const int64_t *ub_prefix, int64_t *c_col_tmp, double *c_val_tmp,
                             int64_t *cnt, void *stream);
int hpcla_spgemm_numeric_i64(int bin, const int64_t *a_rowptr, const int64_t *a_col, const double *a_val,
                             int index_base, const int64_t *g_rowptr, const int64_t *g_col,
                             const double *g_val, const int32_t *row_list, int64_t n_list,
                             const int64_t *ub_prefix, int64_t *c_col_tmp, double *c_val_tmp,
                             int64_t *cnt, void *stream);
int hpcla_spgemm_compact(const int64_t *c_rowptr, const int64_t *ub_prefix, int64_t nrows,
                         const int64_t *c_col_tmp, const double *c_val_tmp, int64_t *c_col, double *c_val,
                         void *stream);
/* Repeated product on a cached structure (the reference recomputes `plan.AT * A_csc` with SparseArrays every time,
 * src/sparse.jl:1011; its MatrixPlan caches the gathering only): result entry e is the sum, in list order, of
 * g_val[pairs[2t + 1]] * a_val[pairs[2t]] for t in [pair_ptr[e], pair_ptr[e + 1]) -- the first product, then the others
 * added one by one (ascending k when the lists are built that way: the bits of hpcla_spgemm_numeric_*).  `pair_ptr` has
 * nnz_c + 1 entries, int32 or int64 (`ptr_is_i64`); `pairs` is 8-byte aligned.  One streaming pass: 8 B per product. */
int hpcla_spgemm_numeric_mapped_f64(const void *pair_ptr, int ptr_is_i64, const int32_t *pairs,
                                    const double *a_val, const double *g_val, double *c_val, int64_t nnz_c,
                                    void *stream);

/* ---- SpMM:  replaces A*B column loop (src/sparse.jl:2391-2413) -------------------------------
 * C[r,c] = sum_j nzval[j] * B[colval[j], c], c in [0,k): one pass over A for all k columns, each
 * (r,c) accumulated sequentially in stored order (bit-identical to k reference SpMVs).
 * B has ncols_compressed rows (or, split form, n_own rows in B_own and ghosts in B_ghost).
 * Fast (16-byte vector) path: row-major B with an EVEN pitch, C row-major on an even pitch or column-major, 16-byte
 * aligned bases.  ODD k takes it too when every row-major pitch is even AND larger than k (ldb = ldc = k + 1 is what the
 * converters of this boundary allocate): the kernel then reads the padding double B[i * ldb + k] of every row it gathers
 * (never stores it), so B / B_ghost must span rows * ldb doubles -- a last row cut off behind its k-th column is not
 * allowed there.  C's padding: with ldc == k + 1 <= 16 the block's C rows leave as whole lines and C[i * ldc + k] is set
 * to 0.0 (a masked last sector per row cost 40 % of the product); any other ldc leaves the padding untouched.  Any other stride combination runs on the generic one-column-per-lane kernel (5-point matrix x 15
 * columns: 0.946 ms on it against 0.475 for 16, profiles/r05_lds_footprint.log). */
int hpcla_spmm_csr_f64_i32(const int32_t *rowptr, const int32_t *colval, const double *nzval,
                           const double *B, int64_t ldb, int b_layout, double *C, int64_t ldc,
                           int c_layout, int64_t nrows, int64_t nnz, int k, int index_base,
                           void *stream);
int hpcla_spmm_csr_f64_i64(const int64_t *rowptr, const int64_t *colval, const double *nzval,
                           const double *B, int64_t ldb, int b_layout, double *C, int64_t ldc,
                           int c_layout, int64_t nrows, int64_t nnz, int k, int index_base,
                           void *stream);
int hpcla_spmm_split_f64_i32(const int32_t *rowptr, const int32_t *colval_split,
                             const double *nzval, const double *B_own, int64_t ldb_own,
                             const double *B_ghost, int64_t ldb_ghost, int64_t n_own, double *C,
                             int64_t ldc, int64_t nrows, int64_t nnz, int k, int index_base,
                             const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmm_split_f64_i64(const int64_t *rowptr, const int64_t *colval_split,
                             const double *nzval, const double *B_own, int64_t ldb_own,
                             const double *B_ghost, int64_t ldb_ghost, int64_t n_own, double *C,
                             int64_t ldc, int64_t nrows, int64_t nnz, int k, int index_base,
                             const int32_t *block_list, int64_t n_blocks, void *stream);
/* hpcla_spmm_split_f64_* with a COLUMN-major result (element (r, c) at C[r + c * ldc], ldc >= nrows; the reference's dense
 * block is a Julia Matrix, src/dense.jl:63) while B_own / B_ghost stay row-major rows: the product an UNSTRUCTURED matrix
 * gets from a column-major caller -- B converted once (hpcla_transpose_f64; an unstructured matrix gathers whole B rows, so
 * the row-major layout is the fast one), C written in the caller's layout by the product itself (the block's results leave
 * through LDS as runs of 64 doubles per column, one launch per 16-column tile; odd k: B pitches even and > k, see above;
 * other pitches: the strided kernel).  Same sums, same order, same bits.
 * hpcla_spmm_csr_f64_* with b_layout = HPCLA_LAYOUT_ROW, c_layout = HPCLA_LAYOUT_COL takes the same kernel. */
int hpcla_spmm_split_ccol_f64_i32(const int32_t *rowptr, const int32_t *colval_split,
                                  const double *nzval, const double *B_own, int64_t ldb_own,
                                  const double *B_ghost, int64_t ldb_ghost, int64_t n_own, double *C,
                                  int64_t ldc, int64_t nrows, int64_t nnz, int k, int index_base,
                                  const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmm_split_ccol_f64_i64(const int64_t *rowptr, const int64_t *colval_split,
                                  const double *nzval, const double *B_own, int64_t ldb_own,
                                  const double *B_ghost, int64_t ldb_ghost, int64_t n_own, double *C,
                                  int64_t ldc, int64_t nrows, int64_t nnz, int k, int index_base,
                                  const int32_t *block_list, int64_t n_blocks, void *stream);
/* RUN TILES (round 4; no reference counterpart -- the reference's A * B is a column loop over A * x,
 * src/sparse.jl:2391-2413): for banded / stencil matrices the 64 rows of an SpMM row block touch a few CONTIGUOUS runs of
 * B rows (5-point matrix: 194 rows in 3 runs, where its entries name 320).  Plan time, once per structure:
 * hpcla_spmm_runs_build_* writes one 32-byte descriptor per block of hpcla_spmm_rows_per_block() rows into `desc`
 * (hpcla_spmm_runs_desc_bytes(nrows) device bytes) -- up to 4 runs {start, length} in the SPLIT column space, cut at the
 * own / ghost boundary; blocks with more runs, more than 200 distinct B rows or more than 512 entries are marked as
 * not fitting -- and returns the number of fitting blocks in *n_fit_host (synchronises the stream).  Per product:
 * hpcla_spmm_runs_k16_f64_* = hpcla_spmm_split_f64_* for k = 16 with ldb_own = ldb_ghost = ldc = 16 (row-major, 16-byte
 * aligned): the runs' B rows are staged into LDS by LDS-DMA next to the block's A entries and multiplied out of LDS in
 * stored order -- bit-identical results, 0.466 ms against 0.517 ms on the 5-point matrix x 16 (0.72 of the HBM peak).
 * Blocks marked as not fitting take a slow per-entry path: use these entries when (nearly) all blocks fit, else the
 * gather kernel.  B_ghost == NULL: every column is owned.  `block_list` as in hpcla_spmm_split_f64_*. */
int64_t hpcla_spmm_runs_desc_bytes(int64_t nrows);
int hpcla_spmm_runs_build_i32(const int32_t *rowptr, const int32_t *colval_split, int64_t nrows, int64_t nnz,
                              int index_base, int64_t n_own, void *desc, int64_t *n_fit_host, void *stream);
int hpcla_spmm_runs_build_i64(const int64_t *rowptr, const int64_t *colval_split, int64_t nrows, int64_t nnz,
                              int index_base, int64_t n_own, void *desc, int64_t *n_fit_host, void *stream);
/* BANDED test of a structure (plan time, one pass, synchronises the stream): the number of hpcla_spmm_rows_per_block()-row
 * blocks whose entries (at most 512) touch at most `max_runs` contiguous runs of split columns, in *n_blocks_host.  Every
 * stencil qualifies (5-point: 3 runs, 7-point: 5); a random pattern has about as many runs as entries.  Column-major callers
 * use it to choose between the product on their blocks as they are (hpcla_spmm_split_colmajor_*: contiguous pieces per gather
 * on a banded structure) and the layout conversions around the row-major kernels. */
int hpcla_spmm_banded_blocks_i32(const int32_t *rowptr, const int32_t *colval_split, int64_t nrows, int64_t nnz,
                                 int index_base, int64_t n_own, int max_runs, int64_t *n_blocks_host, void *stream);
int hpcla_spmm_banded_blocks_i64(const int64_t *rowptr, const int64_t *colval_split, int64_t nrows, int64_t nnz,
                                 int index_base, int64_t n_own, int max_runs, int64_t *n_blocks_host, void *stream);
int hpcla_spmm_runs_k16_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                const double *B_own, const double *B_ghost, int64_t n_own, double *C, int64_t nrows,
                                int64_t nnz, int index_base, const void *desc, const int32_t *block_list,
                                int64_t n_blocks, void *stream);
int hpcla_spmm_runs_k16_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                const double *B_own, const double *B_ghost, int64_t n_own, double *C, int64_t nrows,
                                int64_t nnz, int index_base, const void *desc, const int32_t *block_list,
                                int64_t n_blocks, void *stream);
/* The run tiles on a COLUMN-major caller's blocks (Julia's Matrix, src/dense.jl:63; round 5): hpcla_spmm_split_colmajor_f64_*
 * for k = 16 with the descriptors of hpcla_spmm_runs_build_* -- B_own (n_own rows, ALWAYS the row count of B_own here, also
 * with B_ghost == NULL) and C column-major with leading dimensions ldb_own / ldc, B_ghost the plan's row-major ghost segment
 * (ldb_ghost >= 16) or NULL.  Every own run is widened to an even first row and an even end so that the 16-byte LDS-DMA
 * applies to a column's run: B_own must be 16-byte aligned and ldb_own even (HPCLA_ERR_UNSUPPORTED otherwise: take
 * hpcla_spmm_split_colmajor_f64_*).  Same sums in the same order, same bits.  `block_list` over blocks of
 * hpcla_spmm_rows_per_block() rows, as in hpcla_spmm_runs_k16_f64_*. */
int hpcla_spmm_runs_colmajor_k16_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                         const double *B_own, int64_t ldb_own, const double *B_ghost, int64_t ldb_ghost,
                                         int64_t n_own, double *C, int64_t ldc, int64_t nrows, int64_t nnz, int index_base,
                                         const void *desc, const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmm_runs_colmajor_k16_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                         const double *B_own, int64_t ldb_own, const double *B_ghost, int64_t ldb_ghost,
                                         int64_t n_own, double *C, int64_t ldc, int64_t nrows, int64_t nnz, int index_base,
                                         const void *desc, const int32_t *block_list, int64_t n_blocks, void *stream);
/* Plan-time block order of hpcla_spmm_runs_colmajor_k16_f64_*, by measurement (the twin of hpcla_spmm_tune_block_order_f64_*,
 * whose launch is the row-major gather kernel): the product's own arguments; the launch is timed under the natural order and
 * groups of 8 / 32 / 128 / 512 row blocks, the fastest stays set for `rowptr` (hpcla_spmm_block_order_hint overrides it),
 * *chosen_group receives it (1 = natural).  C receives the product.  Synchronises the stream; launches of fewer than 4096
 * blocks are run once and keep the natural order. */
int hpcla_spmm_runs_colmajor_tune_block_order_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                                      const double *B_own, int64_t ldb_own, const double *B_ghost,
                                                      int64_t ldb_ghost, int64_t n_own, double *C, int64_t ldc, int64_t nrows,
                                                      int64_t nnz, int index_base, const void *desc, const int32_t *block_list,
                                                      int64_t n_blocks, void *stream, int *chosen_group);
int hpcla_spmm_runs_colmajor_tune_block_order_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                                      const double *B_own, int64_t ldb_own, const double *B_ghost,
                                                      int64_t ldb_ghost, int64_t n_own, double *C, int64_t ldc, int64_t nrows,
                                                      int64_t nnz, int index_base, const void *desc, const int32_t *block_list,
                                                      int64_t n_blocks, void *stream, int *chosen_group);
/* A * B on the CALLER's column-major blocks (Julia's Matrix, src/dense.jl:63), no layout conversion (csrc/colmajor.hip):
 * lanes = rows, so the 64 rows of a wave read one contiguous run of a column per gather instruction wherever the matrix is
 * banded; same bits as the row-major kernels.  hpcla_spmm_csr_f64_* takes this path by itself when both layouts are
 * HPCLA_LAYOUT_COL.  Split form: B_own (n_own rows) and C (nrows rows) column-major with leading dimensions ldb_own / ldc;
 * B_ghost is the halo plan's ordinary ROW-major ghost segment (ldb_ghost >= k doubles per ghost row) or NULL; block_list
 * over blocks of hpcla_spmv_rows_per_block() rows.  For unstructured matrices column-major costs a line per (entry, column)
 * pair: convert to row-major rows there (hpcla_transpose_f64) and use hpcla_spmm_split_f64_*. */
int hpcla_spmm_split_colmajor_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                      const double *B_own, int64_t ldb_own, const double *B_ghost, int64_t ldb_ghost,
                                      int64_t n_own, double *C, int64_t ldc, int64_t nrows, int64_t nnz, int k,
                                      int index_base, const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmm_split_colmajor_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                      const double *B_own, int64_t ldb_own, const double *B_ghost, int64_t ldb_ghost,
                                      int64_t n_own, double *C, int64_t ldc, int64_t nrows, int64_t nnz, int k,
                                      int index_base, const int32_t *block_list, int64_t n_blocks, void *stream);
/* hpcla_halo_begin for an operand in any layout (element (row i, column c) at x[i * x_rs + c * x_cs]; a column-major
 * block: x_rs = 1, x_cs = ld): the rows the plan SENDS are staged into `stage` (row-major like the exchange: at least
 * (largest send index + 1) * width doubles, the caller's, reused from call to call) on `stream`, then the ordinary
 * exchange is posted from `stage`.  hpcla_halo_end / status / ghost pointer as usual. */
int hpcla_halo_begin_strided_f64(hpcla_halo_plan_t *plan, const double *x, int64_t x_rs, int64_t x_cs, double *stage,
                                 void *stream);
/* layout conversion for column-major callers (Julia Matrix): dst(row-major, ld=k) <- src */
/* One column PANEL of a product in panel order (opt-in order of the distributed SpMM; the reference's column loop
 * src/sparse.jl:2391-2413 runs one exchange + SpMV per column instead).  (rowptr, colval_split, nzval) hold the
 * entries of A whose columns lie in the panel, in stored order; columns < n_own index B_own, the others B_ghost
 * (n_own = 0: every column is a ghost position).  accumulate = 1: every C(r, c) continues from its current value,
 * entry by entry -- a product taken panel by panel is the reference's sum in a different ORDER (1e-12 relative,
 * not bit-identical).  Row-major B / C (ldb, ldc = row strides). */
int hpcla_spmm_panel_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                             const double *B_own, int64_t ldb_own, const double *B_ghost, int64_t ldb_ghost,
                             int64_t n_own, double *C, int64_t ldc, int64_t nrows, int64_t nnz, int k,
                             int index_base, int accumulate, void *stream);
int hpcla_spmm_panel_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                             const double *B_own, int64_t ldb_own, const double *B_ghost, int64_t ldb_ghost,
                             int64_t n_own, double *C, int64_t ldc, int64_t nrows, int64_t nnz, int k,
                             int index_base, int accumulate, void *stream);
int hpcla_transpose_f64(const double *src, int64_t ld_src, int src_layout, double *dst,
                        int64_t ld_dst, int dst_layout, int64_t rows, int64_t cols, void *stream);

/* ---- dense mat-vec: replaces `LinearAlgebra.mul!(y.v, A.A, plan.gathered)` of
 * Base.:*(A::HPCMatrix, x::HPCVector) / mul! (src/dense.jl:614-658).  A: this rank's rows, ROW-major
 * with leading dimension lda >= ncols; the full x is read in place as three segments (slices owned by
 * lower ranks | own slice | slices of higher ranks), as delivered by a halo plan in which every rank
 * sends its whole slice to every other rank.  Summation order is a tree (BLAS order is
 * implementation-defined): parity by tolerance. */
int hpcla_gemv_rowmajor_f64(const double *A, int64_t lda, int64_t nrows, const double *x_lo, int64_t n_lo,
                            const double *x_own, int64_t n_own, const double *x_hi, int64_t n_hi,
                            double *y, void *stream);
/* transpose(A) * x for the dense row-partitioned A (Base.:*(At::Transpose{T,HPCMatrix}, x),
 * src/dense.jl:1210-1261): y_full[j] = sum_i A[i*lda + j] * x[i] over the LOCAL rows, all ncols
 * columns (the per-rank partial the reference all-reduces: follow with hpcla_allreduce_f64 and keep the
 * own column slice).  x is the slice of the vector on A's ROW partition.  `work`: device scratch of
 * hpcla_gemv_t_work_bytes(nrows, ncols) bytes.  Deterministic two-stage column sums. */
int64_t hpcla_gemv_t_work_bytes(int64_t nrows, int64_t ncols);
int hpcla_gemv_t_rowmajor_f64(const double *A, int64_t lda, int64_t nrows, int64_t ncols, const double *x,
                              double *y_full, void *work, void *stream);

/* transpose(X) * Y of two dense row-partitioned blocks (Base.:*(At::TransposedHPCMatrix, Bmat::HPCMatrix),
 * src/dense.jl:1286-1310): C[i*k + j] = sum over the nrows LOCAL rows r of X[r][i] * Y[r][j], C an m x k ROW-major
 * array of doubles.  X (nrows x m) and Y (nrows x k) are each HPCLA_LAYOUT_ROW (leading dimension >= the width) or
 * HPCLA_LAYOUT_COL (leading dimension >= nrows).  comm NULL: the local partial only; else C is all-reduced in place
 * (one m*k sum through RCCL or the peer window) and a rank with nrows == 0 contributes zeros.  Deterministic: fixed
 * row chunks (a function of nrows, m, k only), one partial tile per chunk, partials summed in a fixed order.  X == Y
 * (non-NULL) with the same layout, leading dimension and m == k: the block is read once and C is exactly symmetric (a
 * rank with nrows == 0 reads neither block: it passes one non-NULL pointer for both when the product is X'X, NULL for
 * both otherwise, so that every rank mirrors the all-reduced C alike).  The f32
 * form widens on load, forms products and sums in double and returns double C (the caller rounds once, after the
 * all-reduce).  work: hpcla_gram_work_bytes(nrows, m, k) bytes of device scratch (host-only function, monotone in
 * nrows).  X and Y aligned to their element size. */
int64_t hpcla_gram_work_bytes(int64_t nrows, int64_t m, int64_t k);
int hpcla_gram_f64(hpcla_comm_t *comm, const double *X, int64_t ldx, int x_layout, const double *Y, int64_t ldy,
                   int y_layout, int64_t nrows, int64_t m, int64_t k, double *C, void *work, void *stream);
int hpcla_gram_f32(hpcla_comm_t *comm, const float *X, int64_t ldx, int x_layout, const float *Y, int64_t ldy,
                   int y_layout, int64_t nrows, int64_t m, int64_t k, double *C, void *work, void *stream);

/* ---- transposed SpMM: W = A^T X for transpose(X) * A and X * A, A sparse (src/sparse.jl:3617-3690) ------------------
 * Structure, once per sparse structure: a local CSC of this rank's rows (rowptr, colval: 0-based CSR over ncols columns,
 * the split column space of the SpMV plan) -- colptr_t (ncols + 1), rowidx_t (nnz: local row, ascending within a column)
 * and perm (nnz: CSC position -> CSR position), in the index type of the inputs.  Stable device sort: equal columns keep
 * their stored order.  work: hpcla_spmm_t_struct_work_bytes(nnz, ncols, index_is_i64) bytes of device scratch (host-only
 * function; -1 on a bad size).
 * Product: W[c, j] = sum over e in [colptr_t[c], colptr_t[c+1]) of nzval[perm[e]] * X[rowidx_t[e], j], j < m, each one
 * running sum from 0.0 in ascending e with separate multiply and add -- the bits of the SpMM over the materialised A^T.  X
 * (the rank's nrows x m block; HPCLA_LAYOUT_ROW is the fast one: one line per entry) and W (ncols x m) each row- or
 * column-major with their leading dimensions.  nzval is read through perm on every call (a matrix with the same structure
 * and new values shares the CSC).  No atomics; the result does not depend on timing.
 * Reverse halo: V[rows[u] * ldv + j] += R[pos[t] * ldr + j] for t in [ptr[u], ptr[u+1]) in list order (int64 lists, u <
 * n_rows, j < m): the owner's own partial plus the partials its peers sent back, in a fixed order. */
int64_t hpcla_spmm_t_struct_work_bytes(int64_t nnz, int64_t ncols, int index_is_i64);
int hpcla_spmm_t_struct_i32(const int32_t *rowptr, const int32_t *colval, int64_t nrows, int64_t nnz, int64_t ncols,
                            int32_t *colptr_t, int32_t *rowidx_t, int32_t *perm, void *work, int64_t work_bytes,
                            void *stream);
int hpcla_spmm_t_struct_i64(const int64_t *rowptr, const int64_t *colval, int64_t nrows, int64_t nnz, int64_t ncols,
                            int64_t *colptr_t, int64_t *rowidx_t, int64_t *perm, void *work, int64_t work_bytes,
                            void *stream);
int hpcla_spmm_t_f64_i32(const int32_t *colptr_t, const int32_t *rowidx_t, const int32_t *perm, const double *nzval,
                         int64_t ncols, const double *X, int64_t ldx, int x_layout, int64_t m, double *W, int64_t ldw,
                         int w_layout, void *stream);
int hpcla_spmm_t_f64_i64(const int64_t *colptr_t, const int64_t *rowidx_t, const int64_t *perm, const double *nzval,
                         int64_t ncols, const double *X, int64_t ldx, int x_layout, int64_t m, double *W, int64_t ldw,
                         int w_layout, void *stream);
int hpcla_spmm_t_accumulate_f64(double *V, int64_t ldv, const double *R, int64_t ldr, const int64_t *rows,
                                const int64_t *ptr, const int64_t *pos, int64_t n_rows, int64_t m, void *stream);

/* ---- gather: replaces _gather_kernel! (src/vectors.jl:174-194) --------------------------------
 * out[dst[i]] = x[src[i]] (dst may be NULL = identity).  The SpMV hot path does not need it (split
 * column space); used for execute_plan! returning `gathered`, the SpGEMM value gather and the value
 * permutations of the TransposePlan (src/sparse.jl:1702-1845). */
int hpcla_gather_f64_i32(const double *x, const int32_t *src, const int32_t *dst, double *out,
                         int64_t n, int index_base, void *stream);
int hpcla_gather_f64_i64(const double *x, const int64_t *src, const int64_t *dst, double *out,
                         int64_t n, int index_base, void *stream);

/* ---- communicator: RCCL over xGMI, replaces comm_* on the hot path (src/backends.jl:264-327)
 * Bootstrap follows ext/HPCLinearAlgebraCUDAExt.jl:388-443: rank 0 gets a 128-byte unique id,
 * the host runtime (MPI.Bcast! / torch.distributed) broadcasts it, every rank calls init_rank.
 * nranks==1 creates a serial communicator that never loads librccl (CommSerial,
 * src/backends.jl:63). */
#define HPCLA_UNIQUE_ID_BYTES 128
int hpcla_comm_get_unique_id(uint8_t *id_host /* 128 bytes */);
int hpcla_comm_init_rank(hpcla_comm_t **comm, const uint8_t *id_host, int nranks, int rank);
/* flags: HPCLA_COMM_NO_RCCL = no RCCL communicator is created (id_host may be NULL); every data-path
 * collective of this communicator then goes through the peer windows below.  Needed where RCCL cannot
 * start -- it refuses two ranks on one GPU ("Duplicate GPU detected"), which is how the multi-rank GPU
 * tests run on a single-GPU box. */
#define HPCLA_COMM_NO_RCCL 1
int hpcla_comm_init_rank_ex(hpcla_comm_t **comm, const uint8_t *id_host, int nranks, int rank, int flags);
int hpcla_comm_rank(const hpcla_comm_t *comm, int *rank);
int hpcla_comm_size(const hpcla_comm_t *comm, int *nranks);
int hpcla_comm_destroy(hpcla_comm_t *comm);
/* in-place all-reduce of `count` doubles on `stream`: op 0 = sum, 1 = max, 2 = product
 * (comm_allreduce(comm, x, + | max | *), src/backends.jl:264-277). */
int hpcla_allreduce_f64(hpcla_comm_t *comm, double *buf, int64_t count, int op, void *stream);

/* ---- peer windows: one-sided transport over xGMI for the ranks of ONE node (csrc/window.hip) --------
 * Replaces, on the hot path, the MPI Isend/Irecv of execute_plan! (src/vectors.jl:431-455) and the scalar
 * comm_allreduce (src/backends.jl:264-277) -- and the RCCL group/all-reduce this library uses otherwise.
 * A window is a fine-grained device allocation that the other ranks map (hipIpcOpenMemHandle) and store
 * into directly; flags/acks in its control lines order producer and consumer, all spins are bounded.
 * Bootstrap is the unique-id pattern again (ext/HPCLinearAlgebraCUDAExt.jl:411-443): every rank EXPORTS a
 * HPCLA_WINDOW_DESC_BYTES descriptor, the host runtime all-gathers them (MPI.Allgather /
 * torch.distributed), every rank ATTACHES.  All ranks must be on one node (descriptor bytes 64..71 hold a
 * node identity the host layer compares before attaching; bytes 112..119 the identity of the GPU that holds
 * the window: attach refuses a peer whose device the runtime reports as not peer-accessible, instead of
 * mapping memory that would fault on the first store).
 *   communicator window: all-reduce of <= 8 doubles in ONE kernel (each rank stores its partial into its
 *     slot of every window, then sums its own window's slots in rank order: the same bits on every rank);
 *   halo plan window:    see hpcla_halo_plan_export below. */
#define HPCLA_WINDOW_DESC_BYTES 128
int hpcla_comm_window_export(hpcla_comm_t *comm, uint8_t *desc_host /* 128 bytes out */);
int hpcla_comm_window_attach(hpcla_comm_t *comm, const uint8_t *all_descs_host /* nranks x 128 bytes */);
/* Connection test after attach: all-reduce of (rank+1) through the windows with its own timeout;
 * *ok = 1 iff it arrived complete.  The host layer all-gathers `ok`; unless every rank passed, every rank
 * calls hpcla_comm_window_detach and the data path stays on RCCL.  Synchronises the device. */
int hpcla_comm_window_selftest(hpcla_comm_t *comm, double timeout_s, int *ok);
int hpcla_comm_window_detach(hpcla_comm_t *comm);
/* 1 in *timed_out if a window all-reduce gave up waiting for a peer (HPCLA_PUSH_TIMEOUT_S, default 300 s: a
 * slow peer is waited for like a blocking MPI_Allreduce, src/backends.jl:264-277; the bound only lets the grid
 * drain when a peer has died).  The result of an expired all-reduce is NaN on this rank.  Synchronises a
 * 4-byte device read. */
int hpcla_comm_status(hpcla_comm_t *comm, int *timed_out);
/* 64-bit identity of (node, physical device): two ranks with equal identities share one GPU. */
int hpcla_device_identity(int device, uint64_t *id);

/* Contiguous-range exchange: device form of execute_plan!(::VectorRepartitionPlan)
 * (src/vectors.jl:624-671; plan lists :511-620), of the dense row repartition (src/dense.jl:1711-1760)
 * and of the nzval leg of the sparse repartition (src/sparse.jl:4443-4535).  For each i < n_send the
 * range src[send_offsets[i] .. +send_counts[i]) goes to send_ranks[i]; for each i < n_recv,
 * recv_counts[i] units from recv_ranks[i] land at dst + recv_offsets[i]; the part that stays
 * (local_src_range / local_dst_offset of the reference plan) is one device copy.  All offsets and
 * counts are 0-based and in units of `width` doubles (1 for vectors and nzval, ncols for row-major
 * dense rows).  Lists are HOST arrays; src/dst are device pointers; one ncclGroup on `stream`. */
int hpcla_exchange_ranges_f64(hpcla_comm_t *comm, const double *src, double *dst, int n_send,
                              const int *send_ranks, const int64_t *send_offsets,
                              const int64_t *send_counts, int n_recv, const int *recv_ranks,
                              const int64_t *recv_offsets, const int64_t *recv_counts,
                              int64_t local_src_offset, int64_t local_dst_offset, int64_t local_count,
                              int width, void *stream);

/* ---- halo plan: device half of VectorPlan / execute_plan! (src/vectors.jl:229-251, 394-463)
 * Inputs are the reference plan's own lists (0-based here):
 *   send_ranks_host[i], send_counts_host[i], send_idx (device, int32 or int64, concatenated in
 *   send_ranks order; local indices into x.v  == plan.send_indices, src/sparse.jl:1939-1944);
 *   recv_ranks_host[i], recv_counts_host[i]: ghost segment i (plan.recv_perm[i]) has
 *   recv_counts[i] entries; segments are stored back to back in recv_ranks order in the ghost
 *   buffer.  Because col_indices is sorted (src/sparse.jl:501) and owners are contiguous rank
 *   ranges (src/sparse.jl:1890), that order IS ascending global column order.
 * `width` = values per index (1 for vectors, k for SpMM ghost rows, row-major).
 * The plan owns: packed send buffer, ghost buffer, one side stream, two events. */
int hpcla_halo_plan_create(hpcla_halo_plan_t **plan, hpcla_comm_t *comm, int n_send,
                           const int32_t *send_ranks_host, const int64_t *send_counts_host,
                           const void *send_idx, int idx_is_i64, int n_recv,
                           const int32_t *recv_ranks_host, const int64_t *recv_counts_host,
                           int width);
/* flags: HPCLA_HALO_SINGLE_BUFFER -- never double-buffer the ghost window.  Required for every plan that is
 * driven through hpcla_halo_begin / hpcla_halo_end with the ghost pointer taken from the host in between
 * (SpMM ghost rows: the interior launch is enqueued before the exchange has completed, so "the buffer of the
 * exchange completed last" is not yet this exchange's buffer); width > 1 plans are single-buffered anyway, the
 * flag matters for a one-column B (width 1).  Vector plans of the fused SpMV keep the default (0). */
#define HPCLA_HALO_SINGLE_BUFFER 1
int hpcla_halo_plan_create_ex(hpcla_halo_plan_t **plan, hpcla_comm_t *comm, int n_send,
                              const int32_t *send_ranks_host, const int64_t *send_counts_host,
                              const void *send_idx, int idx_is_i64, int n_recv,
                              const int32_t *recv_ranks_host, const int64_t *recv_counts_host,
                              int width, int flags);
/* Chain `plan` behind `leader`: both exchange on the LEADER's side stream, so exchanges begun one after the other
 * (hpcla_halo_begin(leader), hpcla_halo_begin(plan), ...) also RUN one after the other -- the chunk-sets of a
 * panel-ordered SpMM arrive in order instead of all at once.  The stream is shared by reference count and goes with
 * the LAST plan of the chain, so the plans may be destroyed in any order. */
int hpcla_halo_plan_chain(hpcla_halo_plan_t *plan, hpcla_halo_plan_t *leader);
int hpcla_halo_plan_destroy(hpcla_halo_plan_t *plan);
/* Push transport for this plan.  When the communicator's window is attached, create() places the ghost
 * segment (double-buffered up to 64 MiB) inside a peer-mappable window.  export: this rank's descriptor
 * plus a table of HPCLA_WINDOW_TABLE_ROWS x nranks int64 (row 0: flag line of source rank r, row 1: offset
 * of r's segment in my ghost, row 2: ack line of consumer rank r, row 3: entries expected from r; -1 =
 * none).  The host runtime all-gathers descriptors and tables; attach maps the neighbours' windows and
 * builds the push lists.  Collective: ranks without neighbours pass a zeroed descriptor / -1 table.
 * After attach, HPCLA_HALO_MODE unset or "push" selects the push transport for this plan. */
#define HPCLA_WINDOW_TABLE_ROWS 4
int hpcla_halo_plan_export(hpcla_halo_plan_t *plan, uint8_t *desc_host, int64_t *table_host);
int hpcla_halo_plan_attach(hpcla_halo_plan_t *plan, const uint8_t *all_descs_host,
                           const int64_t *all_tables_host);
/* give up the push transport of this plan (some rank failed to attach): RCCL receives into the ghost */
int hpcla_halo_plan_detach(hpcla_halo_plan_t *plan);
/* Connection test of one plan on the real topology, run by the host runtime right after attach (collective
 * among the ranks that hold a plan: each makes the same TWO exchanges, one per ghost buffer of a
 * double-buffered plan).  The exchanged vector is x[i*width + j] = rank * 2^40 + i*width + j (+ 0.25 in
 * round two; `n_local_rows` rows); afterwards ghost slot check_slots[t] must hold row check_rows[t] of the
 * rank whose segment the slot lies in (the host knows both from the reference plan: recv_perm and the
 * x partition, src/sparse.jl:1938-1953).  *ok = 1: every checked value arrived and nothing timed out;
 * *ok = 0: hpcla_last_error() says what failed -- the runtime then all-gathers the verdicts and detaches
 * the plan on every rank (hpcla_halo_plan_detach), leaving it on RCCL.  Works for RCCL plans too. */
int hpcla_halo_plan_probe(hpcla_halo_plan_t *plan, int64_t n_local_rows, const int64_t *check_slots_host,
                          const int64_t *check_rows_host, int64_t n_check, void *stream, int *ok);
/* 1 in *timed_out if a push or wait of this plan gave up; synchronising 4-byte read.  An expired WAIT poisons
 * what it would have fed: the waiting row blocks' y entries and dot partials (fused SpMV) or the whole ghost
 * buffer (hpcla_halo_end) become NaN, so the failure cannot pass as a result; an expired ack wait of a PUSH
 * stores nothing and publishes nothing (the consumer may still be reading the buffer).  The status is sticky:
 * the plan is dead afterwards. */
int hpcla_halo_status(hpcla_halo_plan_t *plan, int *timed_out);
/* device pointer of the ghost buffer of the exchange completed last (n_ghost*width doubles) and its length in
 * indices.  Constant for RCCL plans, for dense (width > 1) push plans and for HPCLA_HALO_SINGLE_BUFFER plans;
 * a double-buffered vector push plan reads its device step counter here, i.e. the call SYNCHRONISES the device
 * and is only meaningful AFTER hpcla_halo_end of the exchange in question -- only the API-parity path
 * (execute_plan!'s `gathered`) asks, the fused SpMV finds its buffer in the kernel.  NEVER inside a collective when
 * ranks are threads of one process (a device-wide wait then covers the other ranks' waiting kernels: round 6 found
 * hpcla_halo_plan_probe stalling that way); plans driven through halo_begin / halo_end should be created with
 * HPCLA_HALO_SINGLE_BUFFER, whose pointer is a constant fetched once at plan time. */
int hpcla_halo_ghost_ptr(hpcla_halo_plan_t *plan, double **ghost, int64_t *n_ghost);
/* begin: after everything already enqueued on `stream`, pack x[send_idx] and post the
 * ncclSend/ncclRecv group on the plan's side stream (tag-21 exchange, src/vectors.jl:431-446).
 * end: make `stream` wait for the exchange.  Work enqueued on `stream` between begin and end
 * (the interior SpMV) overlaps the exchange.  x has leading dimension `width` (row-major). */
int hpcla_halo_begin(hpcla_halo_plan_t *plan, const double *x, void *stream);
int hpcla_halo_end(hpcla_halo_plan_t *plan, void *stream);

/* Fused distributed SpMV  y = A*x  (Base.:*(A,x), src/sparse.jl:2096-2128; mul!, :2019-2037).
 * Three orderings, chosen by the environment variable HPCLA_HALO_MODE when the library is first used:
 *   "push"   (default when the plan's peer windows are attached) a push kernel stores the boundary
 *                       values into the neighbours' ghost windows, then ONE launch = interior blocks
 *                       followed by the boundary blocks, which wait in-kernel for the neighbours' flags;
 *                       interior_blocks + boundary_blocks must cover every row block;
 *   "serial" (default otherwise) the RCCL send/recv group on `stream`, then ONE launch over all row blocks;
 *   "overlap"           exchange + boundary blocks on the plan's side stream, interior blocks on
 *                       `stream`, joined by events (block lists from hpcla_classify_blocks_*).
 * On MI355X the SpMV kernel fills every wave slot of every CU, so a side-stream RCCL kernel only runs
 * once the interior grid drains; measured "overlap" = +29..32 us, "serial" = +13..14 us per 4096^2 step
 * (profiles/r01_halo_mode_experiments.log).  Both give the same bits.  With plan==NULL or no
 * neighbours it is a plain split SpMV. */
/* Run-time override of HPCLA_HALO_MODE for plans used from now on: -1 automatic (push where attached,
 * else serial), 0 serial, 1 overlap, 2 push.  Must be called with the same value on every rank, between
 * steps (used by bench.py to time every ordering in one run). */
int hpcla_set_halo_mode(int mode);
int hpcla_spmv_dist_f64_i32(hpcla_halo_plan_t *plan, const int32_t *rowptr,
                            const int32_t *colval_split, const double *nzval, const double *x,
                            int64_t n_own, double *y, int64_t nrows, int64_t nnz, int index_base,
                            const int32_t *interior_blocks, int64_t n_interior,
                            const int32_t *boundary_blocks, int64_t n_boundary, void *stream);
int hpcla_spmv_dist_f64_i64(hpcla_halo_plan_t *plan, const int64_t *rowptr,
                            const int64_t *colval_split, const double *nzval, const double *x,
                            int64_t n_own, double *y, int64_t nrows, int64_t nnz, int index_base,
                            const int32_t *interior_blocks, int64_t n_interior,
                            const int32_t *boundary_blocks, int64_t n_boundary, void *stream);

/* Fused y = A*x and out = x.y (CG's p.Ap; SURVEY section 7 step 6 "SpMV+dot fusion"): the SpMV
 * workgroups leave one partial per row block in `work` (hpcla_spmv_dot_work_bytes(nrows) bytes),
 * summed in index order (deterministic) and all-reduced over `comm` into out_dev[0].
 * Requires x partitioned like A's rows (n_own == nrows). */
int64_t hpcla_spmv_dot_work_bytes(int64_t nrows);
int hpcla_spmv_dist_dot_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                const int32_t *colval_split, const double *nzval, const double *x,
                                int64_t n_own, double *y, int64_t nrows, int64_t nnz, int index_base,
                                const int32_t *interior_blocks, int64_t n_interior,
                                const int32_t *boundary_blocks, int64_t n_boundary,
                                double *dot_out_dev, void *work, void *stream);
int hpcla_spmv_dist_dot_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                const int64_t *colval_split, const double *nzval, const double *x,
                                int64_t n_own, double *y, int64_t nrows, int64_t nnz, int index_base,
                                const int32_t *interior_blocks, int64_t n_interior,
                                const int32_t *boundary_blocks, int64_t n_boundary,
                                double *dot_out_dev, void *work, void *stream);

/* ---- 16-bit block-relative columns: the plan's own narrow copy of the column stream (no reference counterpart: the
 * reference streams colval as stored, src/sparse.jl:2055-2066) ---------------------------------------------------------
 * colval_split is a plan-time copy keyed by the STRUCTURE (src/sparse.jl:1875-1984 builds it once per (A, x.partition)),
 * so the library may store it in any width that holds it -- the step that narrows Int64 to Int32 above, taken once more.
 * For every row block of hpcla_spmv_rows_per_block() = 256 rows whose columns are all owned (< n_own) and lie within
 * [r0 - 32768, r0 + 32767] of the block's first row r0, cols16[j] = colval_split[j] - index_base - r0 as int16: the SpMV
 * then streams 10 instead of 12 bytes per stored entry (2-D 5-point 4096^2: 1.342 GB -> 1.174 GB per product), nzval is
 * read LIVE from the caller's array on every call (unlike the packed copy below, nothing of the values is kept), and y
 * has the same bits: indices are never results.  Cost: 2 bytes of device memory per stored entry and plan.
 *   padded_len: entries the copy must hold for nnz stored entries (a whole number of 8-entry vectors plus one, so that
 *               every aligned 16-byte load of the kernel stays inside the allocation); the buffer must be 16-byte aligned.
 *   encode:     fills the copy for the listed row blocks (block_list == NULL: all; a plan with neighbours lists its
 *               INTERIOR blocks), zeroes every other entry and the pad, and leaves *ineligible_dev (device int) != 0 when
 *               a listed block has a ghost column or a column outside the window: the copy is then not to be used.
 *   spmv_cols16:           y = A*x over the listed (or all) row blocks, every one of which must have been encoded.
 *   spmv_dist_cols16 / spmv_dist_dot_cols16: hpcla_spmv_dist_f64_i32 / hpcla_spmv_dist_dot_f64_i32 with the interior blocks
 *               (no neighbours: all blocks) through the narrow kernel and the boundary blocks through the Int32 kernel;
 *               a contiguous interior run is addressed by its base.  Under the push transport the step is push kernel,
 *               interior launch, waiting boundary launch instead of one fused grid.  cols16 == NULL, a copy that is not
 *               16-byte aligned or nzval that is not 32-byte aligned: exactly the Int32 entry points.
 *   tune_block_order_cols16: hpcla_spmv_tune_block_order_f64_i32 timing the NARROW kernel, the form such a plan launches,
 *               over all blocks (block_base < 0) or over the contiguous run of n_blocks encoded blocks from block_base.
 * Int32 plans (narrowed Int64 plans included), Float64. */
int64_t hpcla_cols16_padded_len(int64_t nnz);
int hpcla_cols16_encode_i32(const int32_t *rowptr, const int32_t *colval_split, int64_t nrows, int64_t nnz, int64_t n_own,
                            int index_base, const int32_t *block_list, int64_t n_blocks, int16_t *cols16,
                            int *ineligible_dev, void *stream);
int hpcla_spmv_cols16_f64_i32(const int32_t *rowptr, const int16_t *cols16, const double *nzval, const double *x, double *y,
                              int64_t nrows, int64_t nnz, int index_base, const int32_t *block_list, int64_t n_blocks,
                              void *stream);
int hpcla_spmv_dist_cols16_f64_i32(hpcla_halo_plan_t *plan, const int32_t *rowptr, const int32_t *colval_split,
                                   const int16_t *cols16, const double *nzval, const double *x, int64_t n_own, double *y,
                                   int64_t nrows, int64_t nnz, int index_base, const int32_t *interior_blocks,
                                   int64_t n_interior, const int32_t *boundary_blocks, int64_t n_boundary, void *stream);
int hpcla_spmv_dist_dot_cols16_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                       const int32_t *colval_split, const int16_t *cols16, const double *nzval,
                                       const double *x, int64_t n_own, double *y, int64_t nrows, int64_t nnz,
                                       int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                       const int32_t *boundary_blocks, int64_t n_boundary, double *dot_out_dev,
                                       void *work, void *stream);
int hpcla_spmv_tune_block_order_cols16_f64_i32(const int32_t *rowptr, const int16_t *cols16, const double *nzval,
                                               const double *x_own, double *y_scratch, int64_t nrows, int64_t nnz,
                                               int index_base, int64_t block_base, int64_t n_blocks, void *stream,
                                               int *chosen_group);

/* ---- repeating block patterns: the column and row-pointer streams of a structured matrix from a table (no reference
 * counterpart: the reference streams rowptr and colval as stored, src/sparse.jl:2055-2066) ---------------------------------
 * A 256-row block has a PATTERN: its row lengths, its block-relative columns (the cols16 copy above) and the position of
 * its first stored entry modulo 8 (the kernel's 16-byte loads start at an 8-entry boundary).  A structured-grid matrix
 * repeats a handful of patterns (2-D 5-point 4096 wide: 18 in 8192 blocks, 46 KB), so a table of them stays in every
 * XCD's L2 and the SpMV no longer streams 2 B per entry of cols16 nor 4 B per row of rowptr from HBM: 8 B per entry of
 * nzval, 16 B per row of x and y and one 8-byte record per block remain (4096^2: 1.174 GB -> 0.940 GB per product).
 * Like cols16 the table is pure STRUCTURE (src/sparse.jl:1875-1984 builds colval_split once per (A, x.partition)):
 * nzval is read live on every call, y has the same bits.
 *   create: hashes every candidate block on the device -- the listed ones, the contiguous run of n_blocks from
 *           block_base (block_list == NULL, block_base >= 0), or all (block_list == NULL, block_base < 0); every one
 *           must have been encoded in cols16 -- counts the hashes on the host, keeps the most frequent patterns up to
 *           256 KiB of table, builds the table from one representative per pattern and compares every block EXACTLY
 *           with its pattern on the device: a block that differs (hash collision), holds more than 65535 entries or
 *           whose pattern was not kept streams cols16 and rowptr as before.  *out == NULL with status 0 when fewer than
 *           half of the candidates ended up in the table (unstructured matrices): launch the cols16 entry points.
 *           HPCLA_BLOCK_PATTERNS_WEAK_HASH leaves the columns out of the hash, so that blocks with equal row lengths
 *           collide: for tests of the exact comparison.  Synchronizes the stream.
 *   info:   kept patterns, bytes of the table, candidate blocks, blocks that read the table.
 *   spmv_patterns / spmv_dist_patterns / spmv_dist_dot_patterns / tune_block_order_patterns: the cols16 entry points of
 *           the same names with the handle; patterns == NULL is exactly those.  The handle must have been created for the
 *           same (nrows, nnz, index_base) and the same rowptr / cols16 contents.  Boundary blocks keep the Int32 kernel. */
#define HPCLA_BLOCK_PATTERNS_WEAK_HASH 1
typedef struct hpcla_block_patterns hpcla_block_patterns_t;
int hpcla_block_patterns_create_i32(hpcla_block_patterns_t **out, const int32_t *rowptr, const int16_t *cols16, int64_t nrows,
                                    int64_t nnz, int index_base, const int32_t *block_list, int64_t block_base,
                                    int64_t n_blocks, int flags, void *stream);
int hpcla_block_patterns_destroy(hpcla_block_patterns_t *p);
int hpcla_block_patterns_info(const hpcla_block_patterns_t *p, int64_t *n_patterns, int64_t *table_bytes,
                              int64_t *n_candidates, int64_t *n_patterned);
int hpcla_spmv_patterns_f64_i32(const int32_t *rowptr, const int16_t *cols16, const hpcla_block_patterns_t *patterns,
                                const double *nzval, const double *x, double *y, int64_t nrows, int64_t nnz, int index_base,
                                const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmv_dist_patterns_f64_i32(hpcla_halo_plan_t *plan, const int32_t *rowptr, const int32_t *colval_split,
                                     const int16_t *cols16, const hpcla_block_patterns_t *patterns, const double *nzval,
                                     const double *x, int64_t n_own, double *y, int64_t nrows, int64_t nnz, int index_base,
                                     const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                                     int64_t n_boundary, void *stream);
int hpcla_spmv_dist_dot_patterns_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                         const int32_t *colval_split, const int16_t *cols16,
                                         const hpcla_block_patterns_t *patterns, const double *nzval, const double *x,
                                         int64_t n_own, double *y, int64_t nrows, int64_t nnz, int index_base,
                                         const int32_t *interior_blocks, int64_t n_interior,
                                         const int32_t *boundary_blocks, int64_t n_boundary, double *dot_out_dev, void *work,
                                         void *stream);
int hpcla_spmv_tune_block_order_patterns_f64_i32(const int32_t *rowptr, const int16_t *cols16,
                                                 const hpcla_block_patterns_t *patterns, const double *nzval,
                                                 const double *x_own, double *y_scratch, int64_t nrows, int64_t nnz,
                                                 int index_base, int64_t block_base, int64_t n_blocks, void *stream,
                                                 int *chosen_group);

/* ---- OPT-IN packed copy of the matrix for SpMV (no reference counterpart) ----------------------------
 * For matrices with <= 256 distinct values whose row blocks reach only columns within +-32 K of the
 * block's first row (stencils, graph Laplacians ...), a plan-time copy with 16-bit block-relative
 * columns and 8-bit value codes moves 3 B per stored entry instead of 12.  The products are the same
 * fp64 numbers summed in the same order, so results stay bit-identical to the CSR path.
 * create returns HPCLA_ERR_UNSUPPORTED when the matrix (restricted to `block_list`, NULL = all row
 * blocks) is not packable.  Int32 indices only.  Reported separately from the CSR numbers. */
typedef struct hpcla_packed hpcla_packed_t;
int hpcla_packed_create_i32(hpcla_packed_t **out, const int32_t *rowptr, const int32_t *colval_split,
                            const double *nzval, int64_t nrows, int64_t nnz, int64_t n_own,
                            int index_base, const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_packed_destroy(hpcla_packed_t *p);
int hpcla_packed_info(const hpcla_packed_t *p, int64_t *bytes, int *ndict);
int hpcla_spmv_packed_f64_i32(const hpcla_packed_t *p, const int32_t *rowptr, const double *x, double *y,
                              int index_base, const int32_t *block_list, int64_t n_blocks,
                              double *dot_partial, void *stream);
/* distributed form of hpcla_spmv_dist_* / hpcla_spmv_dist_dot_* (dot_out_dev may be NULL): interior
 * row blocks from the packed copy, boundary row blocks (ghost columns) from the CSR arrays. */
int hpcla_spmv_dist_packed_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const hpcla_packed_t *p,
                                   const int32_t *rowptr, const int32_t *colval_split,
                                   const double *nzval, const double *x, int64_t n_own, double *y,
                                   int64_t nrows, int64_t nnz, int index_base,
                                   const int32_t *interior_blocks, int64_t n_interior,
                                   const int32_t *boundary_blocks, int64_t n_boundary,
                                   double *dot_out_dev, void *work, void *stream);

/* ---- reductions: replace dot / norm (src/vectors.jl:798-812, 758-780) --------------------------
 * Local deterministic two-stage reduction into out_dev[0] (device double), then, if comm has
 * more than one rank, an in-place RCCL all-reduce on the same stream.  No host sync: CG keeps the
 * scalar on the device.  `work` is a caller-provided device scratch of hpcla_reduce_work_bytes().
 *  dot:   sum x[i]*y[i]
 *  nrm2sq: sum x[i]^2 (the reference squares the local 2-norm before summing, :764-765; the
 *          caller takes sqrt), asum: sum |x[i]| (p=1), amax: max |x[i]| (p=Inf). */
int64_t hpcla_reduce_work_bytes(void);
int hpcla_dot_f64(hpcla_comm_t *comm, const double *x, const double *y, int64_t n, double *out_dev,
                  void *work, void *stream);
int hpcla_nrm2sq_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev, void *work,
                     void *stream);
int hpcla_asum_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev, void *work,
                   void *stream);
int hpcla_amax_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev, void *work,
                   void *stream);
/* maximum(v) (negate = 0) / minimum(v) (negate = 1: out = max(-x), the caller flips the sign)
 * (src/vectors.jl:815-836); an empty vector contributes -inf like typemin in the reference */
int hpcla_maxval_f64(hpcla_comm_t *comm, const double *x, int64_t n, int negate, double *out_dev, void *work,
                     void *stream);
/* sum(v) (src/vectors.jl:838-845): out = sum of all elements over all ranks */
int hpcla_sum_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev, void *work, void *stream);
/* prod(v), src/vectors.jl:853-858 (an empty local part contributes 1) */
int hpcla_prod_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev, void *work, void *stream);
/* general p-norm, p > 0 finite: out = sum |x_i|^p over all ranks; the caller takes the 1/p power
 * (norm(v, p), src/vectors.jl:774-779) */
int hpcla_powsum_f64(hpcla_comm_t *comm, const double *x, int64_t n, double p, double *out_dev, void *work,
                     void *stream);

/* ---- vector updates: replace u+v, a*v and fused broadcast (src/vectors.jl:868-903, 944-964,
 * 1203-1226).  The scalar is alpha_host * (num_dev ? *num_dev : 1) / (den_dev ? *den_dev : 1),
 * so CG coefficients computed by the reductions above never visit the host.
 *  axpy: y[i] = y[i] + a*x[i]      xpay: y[i] = x[i] + a*y[i]
 *  scale: y[i] = a*x[i]            axpby: z[i] = a*x[i] + b*y[i] (host scalars)
 *  divide: y[i] = x[i] / a  (v / a, src/vectors.jl:960-964; a true division, not a reciprocal) */
int hpcla_axpy_f64(double alpha_host, const double *num_dev, const double *den_dev, const double *x,
                   double *y, int64_t n, void *stream);
int hpcla_xpay_f64(const double *x, double alpha_host, const double *num_dev, const double *den_dev,
                   double *y, int64_t n, void *stream);
int hpcla_scale_f64(double alpha_host, const double *x, double *y, int64_t n, void *stream);
/* Fused CG update (two broadcasts + one norm of the reference, src/vectors.jl:1203-1226, 758-765):
 * a = alpha_host * *num_dev / *den_dev;  x += a*p;  r -= a*Ap;  rr_out_dev[0] = allreduce(sum r^2).
 * `work` as for the reductions (hpcla_reduce_work_bytes()). */
int hpcla_cg_update_f64(hpcla_comm_t *comm, double alpha_host, const double *num_dev,
                        const double *den_dev, const double *p, const double *Ap, double *x, double *r,
                        int64_t n, double *rr_out_dev, void *work, void *stream);
/* The same iteration with the x update deferred to the direction update (p is then read once per iteration
 * instead of twice; identical operations per element, identical bits):
 *   residual:  a = alpha_host * *num_dev / *den_dev;  r -= a*Ap;  rr_out_dev[0] = allreduce(sum r^2)
 *   direction: a = alpha_host * *a_num_dev / *a_den_dev, b = beta_host * *b_num_dev / *b_den_dev;
 *              x += a*p;  p = r + b*p      (null num/den pointers count as 1) */
int hpcla_cg_residual_f64(hpcla_comm_t *comm, double alpha_host, const double *num_dev, const double *den_dev,
                          const double *Ap, double *r, int64_t n, double *rr_out_dev, void *work, void *stream);
int hpcla_cg_direction_f64(double alpha_host, const double *a_num_dev, const double *a_den_dev, double beta_host,
                           const double *b_num_dev, const double *b_den_dev, const double *r, double *x,
                           double *p, int64_t n, void *stream);
/* `iters` fused CG iterations enqueued by ONE host call (no reference counterpart: the reference has no
 * Krylov solver, a caller composes the iteration from A*p src/sparse.jl:2096-2128, dot src/vectors.jl:798-812,
 * the broadcasts :1203-1226 and norm :758-765 -- SURVEY 3.4).  Per iteration exactly the launches of
 * hpcla_spmv_dist_dot_* (Ap = A*p, pAp), hpcla_cg_residual_f64 and hpcla_cg_direction_f64, with the same
 * arguments, so the same bits as the three separate calls; neither Python nor Julia sits in the loop.
 * rr_hist_dev: iters + 1 doubles, [0] = sum r_0^2 on entry, [j] = sum r_j^2 on return (device memory; the
 * caller takes the square roots).  pAp_dev: 1 double.  dot_work: hpcla_spmv_dot_work_bytes(nrows) bytes,
 * reduce_work: hpcla_reduce_work_bytes() bytes.  x, r, p, Ap partitioned like A's rows (nrows entries,
 * 16-byte aligned); plan / comm / block lists as for hpcla_spmv_dist_dot_*.  Only enqueues: capturable. */
int hpcla_cg_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                const int32_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                const int32_t *boundary_blocks, int64_t n_boundary, double *x, double *r,
                                double *p, double *Ap, double *rr_hist_dev, double *pAp_dev, void *dot_work,
                                void *reduce_work, int iters, void *stream);
int hpcla_cg_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                const int32_t *boundary_blocks, int64_t n_boundary, double *x, double *r,
                                double *p, double *Ap, double *rr_hist_dev, double *pAp_dev, void *dot_work,
                                void *reduce_work, int iters, void *stream);
/* ---- a converging CG solver: gated, diagonally preconditioned iterations (no reference counterpart: the reference's
 * only solver is MUMPS on the host).  The solve's state is device memory, so the host looks once per chunk of
 * iterations and the iterations already enqueued behind the deciding one are no-ops:
 *   state_dev[0] done_iter  the iteration the solve ended on (meaningful once status != 0)
 *   state_dev[1] status     0 running, 1 converged, 2 breakdown
 *   state_dev[2] thr        a double: max(rtol |b|, atol)^2, written by the caller       state_dev[3] reserved
 * Iteration `iter` is 1-based over the whole solve.
 *   residual:  while status == 0.  !(*den_dev > 0) (pAp; catches NaN): status = 2, done_iter = iter - 1, nothing else
 *              written.  Else a = *num_dev / *den_dev;  r -= a*Ap;  pair_out_dev[0] = allreduce(sum r^2),
 *              pair_out_dev[1] = allreduce(sum r*(dinv*r)) -- ONE all-reduce of the two doubles;  then
 *              pair_out_dev[0] <= thr: status = 1, done_iter = iter.
 *   direction: while status == 0, and once more when status == 1 and done_iter >= iter (the x update of the converging
 *              iteration is deferred into it).  a = *a_num_dev / *a_den_dev, b = *b_num_dev / *b_den_dev;
 *              x += a*p;  p = dinv*r + b*p   (z = dinv*r is never stored).
 * dinv == NULL is the identity: no load, no multiply, and the bits of hpcla_cg_residual_f64 / hpcla_cg_direction_f64 on
 * the same operands (same grid, body, tail, accumulation order, HPCLA_CG_NT policy).  Separate multiply and add.
 * work: hpcla_pcg_work_bytes() bytes -- two arrays of partials, then 32 bytes that hpcla_pcg_iterations_* uses as the
 * state (at work + hpcla_pcg_work_bytes() - 32).  Vectors 16-byte aligned. */
int64_t hpcla_pcg_work_bytes(void);
int hpcla_pcg_residual_f64(hpcla_comm_t *comm, const double *num_dev, const double *den_dev, const double *Ap,
                           const double *dinv, double *r, int64_t n, int64_t iter, int64_t *state_dev,
                           double *pair_out_dev, void *work, void *stream);
int hpcla_pcg_direction_f64(const double *a_num_dev, const double *a_den_dev, const double *b_num_dev,
                            const double *b_den_dev, const double *r, const double *dinv, double *x, double *p,
                            int64_t n, int64_t iter, const int64_t *state_dev, void *stream);
/* Iterations first_iter .. first_iter + iters - 1 of that solve enqueued by ONE host call: per iteration
 * hpcla_spmv_dist_dot_* (Ap = A*p, pAp; always executed), hpcla_pcg_residual_f64 (num = rz_{j-1}, den = pAp) and
 * hpcla_pcg_direction_f64 (b = rz_j / rz_{j-1}).  hist_dev: pairs, [2j] = sum r_j^2 and [2j+1] = sum r_j*(dinv*r_j);
 * pair 0 on entry of the first chunk, pair j written by iteration j; pairs beyond done_iter are unspecified.  The state
 * (see above) lives in the last 32 bytes of pcg_work and is set up by the caller.  cols16 / patterns: the plan's 16-bit
 * column copy and pattern table as for hpcla_spmv_dist_dot_patterns_f64_i32, NULL allowed.  Everything else as for
 * hpcla_cg_iterations_*.  Only enqueues. */
int hpcla_pcg_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                 const int32_t *colval_split, const int16_t *cols16,
                                 const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows,
                                 int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                 const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, double *x,
                                 double *r, double *p, double *Ap, double *hist_dev, double *pAp_dev, void *dot_work,
                                 void *pcg_work, int64_t first_iter, int iters, void *stream);
int hpcla_pcg_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                 const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                 int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                 const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, double *x,
                                 double *r, double *p, double *Ap, double *hist_dev, double *pAp_dev, void *dot_work,
                                 void *pcg_work, int64_t first_iter, int iters, void *stream);
/* ---- factorised sparse approximate inverse (hp.fsai; csrc/fsai.hip): a sparse lower triangular G with diag(G A G') = 1 on a
 * given pattern, M = G' G as the preconditioner of the CG solver above (no reference counterpart: the reference's only
 * solver is MUMPS on the host, and it has no preconditioner).  Rows and columns of A are partitioned alike (n_own == nrows), so
 * a split column < n_own is the local row it names; columns >= n_own are ghosts and are skipped: G couples a rank's own rows
 * only.  Row i of G lives on J_i = the pattern columns < i of row i, ascending, then i (m = |J_i| <= 32): with S = A[J_i, J_i]
 * (an unstored entry is 0, only the lower triangle is read) and S = L L', the row is inv(L') e_m.  p_* is the pattern's
 * structure, a_* the matrix; they may be the same arrays.
 *   fsai_work_bytes  device bytes of `work` for the count.
 *   fsai_count       g_rowptr_dev: nrows + 1 entries, 0-based.  info_dev[0] = nnz(G), info_dev[1] = the largest m,
 *                    info_dev[2] = the error word, reset here: all ones, or (local row << 2) | code of the smallest failing
 *                    row -- 1: m > 32, 2: A stores no diagonal in the row, 3: a pivot of S that is not > 0 (NaN included).
 *   fsai_factor      max_m: at least the largest m of the count (selects 4, 8, 16 or 32 lanes per row).  Writes G's global
 *                    column ids (col_start + local column) and values at g_rowptr_dev's positions; a failing row gets zeros
 *                    and lowers the error word.  The bits of a row do not depend on max_m, the launch or the call.
 * Both only enqueue (vector atomic min / max on info_dev, no waiting). */
int64_t hpcla_fsai_work_bytes(int64_t nrows);
int hpcla_fsai_count_f64_i32(const int32_t *p_rowptr, const int32_t *p_colval_split, const int32_t *a_rowptr,
                             const int32_t *a_colval_split, int64_t nrows, int64_t n_own, int index_base,
                             int64_t *g_rowptr_dev, int64_t *info_dev, void *work, void *stream);
int hpcla_fsai_count_f64_i64(const int64_t *p_rowptr, const int64_t *p_colval_split, const int64_t *a_rowptr,
                             const int64_t *a_colval_split, int64_t nrows, int64_t n_own, int index_base,
                             int64_t *g_rowptr_dev, int64_t *info_dev, void *work, void *stream);
int hpcla_fsai_factor_f64_i32(const int32_t *p_rowptr, const int32_t *p_colval_split, const int32_t *a_rowptr,
                              const int32_t *a_colval_split, const double *a_nzval, int64_t nrows, int64_t n_own,
                              int index_base, int64_t col_start, int max_m, const int64_t *g_rowptr_dev,
                              int64_t *g_cols_dev, double *g_vals_dev, int64_t *info_dev, void *stream);
int hpcla_fsai_factor_f64_i64(const int64_t *p_rowptr, const int64_t *p_colval_split, const int64_t *a_rowptr,
                              const int64_t *a_colval_split, const double *a_nzval, int64_t nrows, int64_t n_own,
                              int index_base, int64_t col_start, int max_m, const int64_t *g_rowptr_dev,
                              int64_t *g_cols_dev, double *g_vals_dev, int64_t *info_dev, void *stream);
/* Iterations of the CG solver with M = Gt G, G and Gt matrices with plans of their own (the three plan / CSR blocks are A's,
 * G's and Gt's, each as for hpcla_pcg_iterations_*): per iteration hpcla_spmv_dist_dot_*, hpcla_pcg_residual_f64 with
 * dinv == NULL, u = G r and z = Gt u through hpcla_spmv_dist_* (always executed), hpcla_nrm2sq_f64 of u into
 * hist_dev[2j+1] (r.M r = sum u^2, never negative; always executed), hpcla_pcg_direction_f64 with z in place of r.  State,
 * history, scratch and stop rule are hpcla_pcg_iterations_*'s.  Only enqueues. */
int hpcla_pcg_fsai_iterations_f64_i32(
    hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int32_t *rowptr, const int32_t *colval_split, const int16_t *cols16,
    const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows, int64_t nnz, int index_base,
    const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks, int64_t n_boundary,
    hpcla_halo_plan_t *plan_g, const int32_t *rowptr_g, const int32_t *colval_split_g, const int16_t *cols16_g,
    const hpcla_block_patterns_t *patterns_g, const double *nzval_g, int64_t nrows_g, int64_t nnz_g, int index_base_g,
    const int32_t *interior_blocks_g, int64_t n_interior_g, const int32_t *boundary_blocks_g, int64_t n_boundary_g,
    hpcla_halo_plan_t *plan_t, const int32_t *rowptr_t, const int32_t *colval_split_t, const int16_t *cols16_t,
    const hpcla_block_patterns_t *patterns_t, const double *nzval_t, int64_t nrows_t, int64_t nnz_t, int index_base_t,
    const int32_t *interior_blocks_t, int64_t n_interior_t, const int32_t *boundary_blocks_t, int64_t n_boundary_t, double *x,
    double *r, double *p, double *Ap, double *u, double *z, double *hist_dev, double *pAp_dev, void *dot_work, void *pcg_work,
    int64_t first_iter, int iters, void *stream);
int hpcla_pcg_fsai_iterations_f64_i64(
    hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
    int64_t nrows, int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
    const int32_t *boundary_blocks, int64_t n_boundary, hpcla_halo_plan_t *plan_g, const int64_t *rowptr_g,
    const int64_t *colval_split_g, const double *nzval_g, int64_t nrows_g, int64_t nnz_g, int index_base_g,
    const int32_t *interior_blocks_g, int64_t n_interior_g, const int32_t *boundary_blocks_g, int64_t n_boundary_g,
    hpcla_halo_plan_t *plan_t, const int64_t *rowptr_t, const int64_t *colval_split_t, const double *nzval_t, int64_t nrows_t,
    int64_t nnz_t, int index_base_t, const int32_t *interior_blocks_t, int64_t n_interior_t, const int32_t *boundary_blocks_t,
    int64_t n_boundary_t, double *x, double *r, double *p, double *Ap, double *u, double *z, double *hist_dev, double *pAp_dev,
    void *dot_work, void *pcg_work, int64_t first_iter, int iters, void *stream);
/* ---- smoothed-aggregation multigrid (hp.amg, csrc/amg.hip): the setup kernels of a level and the two fused smoother updates
 * of the cycle (no reference counterpart).  The setup's products, its transpose and the cycle's SpMVs are the entries above.
 * Rows and columns of A are partitioned alike (n_own == nrows < 2^31): a split column < n_own is the local row it names, columns
 * >= n_own are ghosts, which the weights read and the strength graph leaves out (aggregates never cross ranks).
 *   amg_work_bytes     device bytes of `work` for the scans.   amg_round_blocks  entries of block_undecided_dev.
 *   amg_weights        diag_dev[i] = a_ii (+0.0 where none is stored), ratio_dev[i] = sum_j |a_ij| / a_ii over the whole row;
 *                      info_dev[0] = all ones, or the smallest local row with !(a_ii > 0) (NaN included).
 *   amg_smoother       s = w ./ diag.
 *   amg_strength_count / _fill   the graph of entries c != i, c < n_own, a_ic != 0, |a_ic| >= theta sqrt(a_ii a_cc), theta in
 *                      [0, 1): s_rowptr_dev (nrows + 1, 0-based), info_dev[0] = its entries; then local columns, row order kept.
 *   amg_mis_init       key = (h(row_start + i) << 31) | i with h the 31-bit mix of csrc/amg.hip; state = key.
 *   amg_mis_round      one round of the distance-2 independent set, three launches: m1, m2 (neighbour maxima of the state: key
 *                      undecided, 2^62 root, -1 out), state_out, and per workgroup the rows still undecided.  No atomics.
 *   amg_join           owner_b_dev[i] = the local row of i's root (pass 1 into owner_a_dev: roots and their neighbours; pass 2:
 *                      the rest), rootid_dev = the exclusive scan of the root flags; info_dev[0] = all ones or a row left
 *                      without a root (cannot happen for a maximal set), info_dev[1] = the number of roots.
 *   amg_aggregate_ids  agg_dev[i] = offset + rootid[owner[i]]: global aggregate ids.
 *   amg_prolongator    p_ic = [c == agg(i)] - s_i * (A T)_ic on the CSR of A T (compressed local columns, their global ids).
 *   amg_presmooth      x = s .* b.      amg_postsmooth  x += s .* (b - t).  16-byte aligned vectors.
 * For a nonsymmetric A (hp.amg(A, symmetric=False)):
 *   amg_symmetrise_count / _fill   the graph E u E^T of the strength graph E (s_rowptr_dev, s_cols_dev): indeg_dev (nrows words)
 *                      = the in-degrees by integer atomics, u_rowptr_dev (nrows + 1) = the scan of out- plus in-degrees,
 *                      info_dev[0] = its entries; then each row's out-list followed by its in-list (cursor_dev: nrows words of
 *                      scratch).  The in-list's order is not defined and an edge stored both ways appears twice; the rounds and
 *                      the join depend on the set of a row's neighbours only.  One index form: the graph's own.
 *   amg_restrictor     r_cj = [agg(j) == row_offset + c] - (T^t A)_cj * s_j on the CSR of T^t A (compressed local columns, their
 *                      global ids, each in 0..ncols and owned): the Petrov-Galerkin restriction T^t (I - A S).
 * With near-nullspace candidates (hp.amg(A, B=...)), 1 <= k <= 8 columns, k coarse unknowns per aggregate (k * agg + c):
 *   amg_fit            per aggregate a (its members: members_dev[member_ptr_dev[a] .. member_ptr_dev[a + 1]), local rows,
 *                      ascending) B[members, :] = Q R: Q into the rows of tv_dev (nrows x k, row-major, as b_dev), R into rows
 *                      k a .. k a + k - 1 of bc_dev (k n_aggregates x k), +0.0 below the diagonal.  Classical Gram-Schmidt run
 *                      twice, every sum by one lane in ascending member order (csrc/amg.hip has the arithmetic, which is part of
 *                      the method's definition).  A column with !(nr > 1e-10 n0) is dropped (q_j = 0, row j of R = 0);
 *                      info_dev[0] = all ones, or 8 a + j of the smallest aggregate that dropped one and its first such column.
 *   amg_prolongator_b  p_e = (col / k == agg(i) ? tv[i, col - k agg(i)] : 0) - s_i * (A T)_e on the CSR of A T.
 *   amg_restrictor_b   r_cj = (agg(j) == (row_offset + c) / k ? tv[j, (row_offset + c) % k] : 0) - (T^t A)_cj * s_j.
 * All only enqueue. */
int hpcla_amg_fit_f64(const double *b_dev, int64_t nrows, int k, const int64_t *member_ptr_dev, const int64_t *members_dev,
                      int64_t n_members, int64_t n_aggregates, double *tv_dev, double *bc_dev, int64_t *info_dev, void *stream);
int hpcla_amg_prolongator_b_f64_i32(const int32_t *at_rowptr, const int32_t *at_colval, const int64_t *at_col_indices_dev,
                                    const double *at_nzval, const int64_t *agg_dev, const double *s_dev, const double *tv_dev, int k,
                                    int64_t nrows, int index_base, double *p_nzval, void *stream);
int hpcla_amg_prolongator_b_f64_i64(const int64_t *at_rowptr, const int64_t *at_colval, const int64_t *at_col_indices_dev,
                                    const double *at_nzval, const int64_t *agg_dev, const double *s_dev, const double *tv_dev, int k,
                                    int64_t nrows, int index_base, double *p_nzval, void *stream);
int hpcla_amg_restrictor_b_f64_i32(const int32_t *ta_rowptr, const int32_t *ta_colval, const int64_t *ta_col_indices_dev,
                                   const double *ta_nzval, const int64_t *agg_dev, const double *s_dev, const double *tv_dev, int k,
                                   int64_t nrows, int64_t ncols, int64_t row_offset, int index_base, double *r_nzval, void *stream);
int hpcla_amg_restrictor_b_f64_i64(const int64_t *ta_rowptr, const int64_t *ta_colval, const int64_t *ta_col_indices_dev,
                                   const double *ta_nzval, const int64_t *agg_dev, const double *s_dev, const double *tv_dev, int k,
                                   int64_t nrows, int64_t ncols, int64_t row_offset, int index_base, double *r_nzval, void *stream);
int64_t hpcla_amg_work_bytes(int64_t nrows);
int64_t hpcla_amg_round_blocks(int64_t nrows);
int hpcla_amg_weights_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval, int64_t nrows,
                              int64_t n_own, int index_base, double *diag_dev, double *ratio_dev, int64_t *info_dev,
                              void *stream);
int hpcla_amg_weights_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval, int64_t nrows,
                              int64_t n_own, int index_base, double *diag_dev, double *ratio_dev, int64_t *info_dev,
                              void *stream);
int hpcla_amg_smoother_f64(double w, const double *diag_dev, double *s_dev, int64_t n, void *stream);
int hpcla_amg_strength_count_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                     const double *diag_dev, int64_t nrows, int64_t n_own, int index_base, double theta,
                                     int64_t *s_rowptr_dev, int64_t *info_dev, void *work, void *stream);
int hpcla_amg_strength_count_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                     const double *diag_dev, int64_t nrows, int64_t n_own, int index_base, double theta,
                                     int64_t *s_rowptr_dev, int64_t *info_dev, void *work, void *stream);
int hpcla_amg_strength_fill_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                    const double *diag_dev, int64_t nrows, int64_t n_own, int index_base, double theta,
                                    const int64_t *s_rowptr_dev, int32_t *s_cols_dev, void *stream);
int hpcla_amg_strength_fill_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                    const double *diag_dev, int64_t nrows, int64_t n_own, int index_base, double theta,
                                    const int64_t *s_rowptr_dev, int32_t *s_cols_dev, void *stream);
int hpcla_amg_mis_init(int64_t nrows, int64_t row_start, int64_t *key_dev, int64_t *state_dev, void *stream);
int hpcla_amg_mis_round(const int64_t *s_rowptr_dev, const int32_t *s_cols_dev, int64_t nrows, const int64_t *key_dev,
                        const int64_t *state_in_dev, int64_t *m1_dev, int64_t *m2_dev, int64_t *state_out_dev,
                        int64_t *block_undecided_dev, void *stream);
int hpcla_amg_join(const int64_t *s_rowptr_dev, const int32_t *s_cols_dev, int64_t nrows, const int64_t *key_dev,
                   const int64_t *state_dev, int32_t *owner_a_dev, int32_t *owner_b_dev, int64_t *rootid_dev, int64_t *info_dev,
                   void *work, void *stream);
int hpcla_amg_aggregate_ids(const int32_t *owner_dev, const int64_t *rootid_dev, int64_t nrows, int64_t offset, int64_t *agg_dev,
                            void *stream);
int hpcla_amg_prolongator_f64_i32(const int32_t *at_rowptr, const int32_t *at_colval, const int64_t *at_col_indices_dev,
                                  const double *at_nzval, const int64_t *agg_dev, const double *s_dev, int64_t nrows,
                                  int index_base, double *p_nzval, void *stream);
int hpcla_amg_prolongator_f64_i64(const int64_t *at_rowptr, const int64_t *at_colval, const int64_t *at_col_indices_dev,
                                  const double *at_nzval, const int64_t *agg_dev, const double *s_dev, int64_t nrows,
                                  int index_base, double *p_nzval, void *stream);
int hpcla_amg_symmetrise_count(const int64_t *s_rowptr_dev, const int32_t *s_cols_dev, int64_t nrows, int64_t *indeg_dev,
                               int64_t *u_rowptr_dev, int64_t *info_dev, void *work, void *stream);
int hpcla_amg_symmetrise_fill(const int64_t *s_rowptr_dev, const int32_t *s_cols_dev, int64_t nrows, const int64_t *u_rowptr_dev,
                              int64_t *cursor_dev, int32_t *u_cols_dev, void *stream);
int hpcla_amg_restrictor_f64_i32(const int32_t *ta_rowptr, const int32_t *ta_colval, const int64_t *ta_col_indices_dev,
                                 const double *ta_nzval, const int64_t *agg_dev, const double *s_dev, int64_t nrows, int64_t ncols,
                                 int64_t row_offset, int index_base, double *r_nzval, void *stream);
int hpcla_amg_restrictor_f64_i64(const int64_t *ta_rowptr, const int64_t *ta_colval, const int64_t *ta_col_indices_dev,
                                 const double *ta_nzval, const int64_t *agg_dev, const double *s_dev, int64_t nrows, int64_t ncols,
                                 int64_t row_offset, int index_base, double *r_nzval, void *stream);
int hpcla_amg_presmooth_f64(const double *s_dev, const double *b, double *x, int64_t n, void *stream);
int hpcla_amg_postsmooth_f64(const double *s_dev, const double *b, const double *t, double *x, int64_t n, void *stream);
/* ---- fine-grained ILU(0) (hp.ilu0, csrc/ilu.hip): Chow-Patel sweeps for the factors, truncated Jacobi sweeps in place of the
 * two triangular solves, as the preconditioner of the GMRES and BiCGStab solvers below (no reference counterpart: the
 * reference's only solver is MUMPS on the host, and it has no preconditioner).  Rows and columns of A are partitioned alike
 * (n_own == nrows < 2^31 - 1), so a split column < n_own is the local row it names; columns >= n_own are ghosts and are dropped:
 * the factors couple a rank's own rows only.  The owned block is a CSR of its own with Int32 indices (fewer than 2^31 entries):
 * b_rowptr_dev (nrows + 1, 0-based), b_cols_dev (local columns, ascending within a row whatever A's order), b_rows_dev (the row
 * of every entry), b_diag_dev (the position of a row's diagonal, -1 when none is stored), b_map_dev (the entry's 0-based
 * position in A's nzval).  c_ptr_dev (nrows + 1) / c_pos_dev: the entries of column j as positions into the block, ascending
 * row -- a stable sort of the positions by column, left to the caller.  f: one value per block entry, l_ij for i > j (unit
 * diagonal not stored), u_ij for i <= j.
 *   ilu_work_bytes  device bytes of `work` for the count.
 *   ilu_count       b_rowptr_dev.  info_dev[0] = the block's entries, info_dev[1] = the error word, reset here: all ones, or
 *                   (local row << 2) | code of the smallest failing row -- 1: the row stores no diagonal, 2: its diagonal is zero
 *                   or NaN, 3: its pivot u_ii is zero, NaN or infinite.
 *   ilu_fill        the other index arrays (an entry's place in its row: the number of owned entries with a smaller column;
 *                   quadratic in the row's length, no scratch); lowers the error word with codes 1 and 2.
 *   ilu_gather      a_vals_dev[p] = a_nzval[b_map_dev[p]]: the block's values, also new values for an unchanged structure.
 *   ilu_init        f = the initial guess: l_ij = a_ij / a_jj, u_ij = a_ij.
 *   ilu_sweep       one lane per entry: s = a_ij - sum_{k < min(i, j), (i, k) and (k, j) stored} l_ik * u_kj from f_old_dev in
 *                   ascending k, multiply and subtract separately rounded; f_new_dev = s / u_jj (f_old_dev's) for i > j, s
 *                   otherwise.  Two buffers; rows of any length; no atomics.  A row without a diagonal yields NaN.
 *   ilu_pivots      dinv_dev[i] = 1 / u_ii; lowers the error word with code 3.
 *   ilu_trisweep    out_i = (rhs_i - sum_p f_p * in[col_p]) [* dinv_i] over the part of row i below (upper == 0) or above
 *                   (upper != 0) its diagonal, in one kernel.  lanes = 1: one lane per row, a running subtraction in stored
 *                   order; 2, 4, 8: a lane group per row, partial sums joined by shuffles, subtracted once.  in == NULL: the
 *                   sum is empty; dinv_dev == NULL: no scaling.  in and out are two buffers.  No alignment is asked for.
 *   ilu_apply       out = N_U(N_L(r)) in 2 solve_sweeps + 1 trisweep launches: y_0 = r, y_{m+1} = r - L y_m;  z_0 = dinv .* y,
 *                   z_{m+1} = dinv .* (y - U z_m), solve_sweeps (1..16) times each.  t0, t1: scratch of nrows doubles, distinct
 *                   from each other, from r and from out.  out may be r: r is last read before out is first written.
 * All only enqueue (vector atomic min on info_dev, no waiting); every result is fixed by the inputs. */
int64_t hpcla_ilu_work_bytes(int64_t nrows);
int hpcla_ilu_count_f64_i32(const int32_t *a_rowptr, const int32_t *a_colval_split, int64_t nrows, int64_t n_own,
                            int index_base, int32_t *b_rowptr_dev, int64_t *info_dev, void *work, void *stream);
int hpcla_ilu_count_f64_i64(const int64_t *a_rowptr, const int64_t *a_colval_split, int64_t nrows, int64_t n_own,
                            int index_base, int32_t *b_rowptr_dev, int64_t *info_dev, void *work, void *stream);
int hpcla_ilu_fill_f64_i32(const int32_t *a_rowptr, const int32_t *a_colval_split, const double *a_nzval, int64_t nrows,
                           int64_t n_own, int index_base, const int32_t *b_rowptr_dev, int32_t *b_cols_dev,
                           int32_t *b_rows_dev, int32_t *b_diag_dev, int64_t *b_map_dev, int64_t *info_dev, void *stream);
int hpcla_ilu_fill_f64_i64(const int64_t *a_rowptr, const int64_t *a_colval_split, const double *a_nzval, int64_t nrows,
                           int64_t n_own, int index_base, const int32_t *b_rowptr_dev, int32_t *b_cols_dev,
                           int32_t *b_rows_dev, int32_t *b_diag_dev, int64_t *b_map_dev, int64_t *info_dev, void *stream);
int hpcla_ilu_gather_f64(const double *a_nzval, const int64_t *b_map_dev, int64_t nnz, double *a_vals_dev, void *stream);
int hpcla_ilu_init_f64(const int32_t *b_cols_dev, const int32_t *b_rows_dev, const int32_t *b_diag_dev,
                       const double *a_vals_dev, int64_t nnz, double *f_dev, void *stream);
int hpcla_ilu_sweep_f64(const int32_t *b_rowptr_dev, const int32_t *b_cols_dev, const int32_t *b_rows_dev,
                        const int32_t *b_diag_dev, const int32_t *c_ptr_dev, const int32_t *c_pos_dev,
                        const double *a_vals_dev, const double *f_old_dev, double *f_new_dev, int64_t nnz, void *stream);
int hpcla_ilu_pivots_f64(const int32_t *b_diag_dev, const double *f_dev, int64_t nrows, double *dinv_dev, int64_t *info_dev,
                         void *stream);
int hpcla_ilu_trisweep_f64(const int32_t *b_rowptr_dev, const int32_t *b_cols_dev, const int32_t *b_diag_dev,
                           const double *f_dev, const double *rhs, const double *in, const double *dinv_dev, double *out,
                           int64_t nrows, int upper, int lanes, void *stream);
int hpcla_ilu_apply_f64(const int32_t *b_rowptr_dev, const int32_t *b_cols_dev, const int32_t *b_diag_dev, const double *f_dev,
                        const double *dinv_dev, const double *r, double *t0, double *t1, double *out, int64_t nrows,
                        int solve_sweeps, int lanes, void *stream);
/* ---- BiCGStab for nonsymmetric A: gated steps of right-preconditioned BiCGStab, K = identity or dinv .* (no reference
 * counterpart: the reference solves a general A \ b through MUMPS on the host; a caller of its operators composes the
 * method from A*p, src/sparse.jl:2096-2128, dot, src/vectors.jl:798-812, and the broadcasts, src/vectors.jl:1203-1226).
 * The state is the CG solver's (done_iter, status, thr, reserved) with one more status:
 *   3 converged at the half step (sum s^2 <= thr at done_iter): x = x + a*ph only, r untouched; callers report "converged".
 * Iteration `iter` is 1-based over the whole solve; every entry is a no-op writing no byte once status != 0 (bicg_xr runs
 * once more, in its half-step form, when status == 3 and done_iter == iter).  a = *rho_dev / *rv_dev, w = ts / tt with
 * triple_dev = (ts, tt, ss), b = (*rho_new_dev / *rho_dev) * (a / w): formed in every kernel from the same doubles.
 * Each reduction is all-reduced once (comm != NULL) and followed by its gates, in this order:
 *   bicg_dot  (stands for dot)              *rv_out_dev = rhat.v.  Gate A: !(rho != 0 && rv != 0), NaN included:
 *                                           status = 2, done_iter = iter - 1.
 *   bicg_s    (one broadcast, two with dinv) s = r - a*v;  sh = dinv .* s when dinv != NULL (sh may be NULL otherwise).  Also
 *                                           a no-op under gate A's predicate.
 *   bicg_tts  (three dots)                  triple_out_dev = (t.s, t.t, s.s), one pass.  Gate S: ss <= thr: status = 3,
 *                                           done_iter = iter.  Gate T: !(tt > 0): status = 2, done_iter = iter - 1.
 *   bicg_xr   (two broadcasts, dot, norm)   x = (x + a*ph) + w*sh;  r = s - w*t;  pair_out_dev = (sum r^2, rhat.r).  sh == NULL
 *                                           means sh is s (the identity).  Gate B: sum r^2 <= thr: status = 1, done_iter =
 *                                           iter.  Gate O: ts == 0: status = 2, done_iter = iter.  In the half-step form
 *                                           pair_out_dev[0] = ss (triple_dev[2]), stored behind the pair's all-reduce so
 *                                           that N ranks do not sum the already global value; pair_out_dev[1] unspecified.
 *   bicg_p    (two broadcasts, three with dinv) p = r + b*(p - w*v);  ph = dinv .* p when dinv != NULL.
 * Separate multiply and add, in the order written.  work: the byte count of hpcla_bicgstab_work_bytes -- three arrays of
 * partials, then the 32 bytes the iterations entry uses as the state.  Vectors 16-byte aligned. */
int64_t hpcla_bicgstab_work_bytes(void);
int hpcla_bicg_dot_f64(hpcla_comm_t *comm, const double *rhat, const double *v, int64_t n, int64_t iter,
                       const double *rho_dev, int64_t *state_dev, double *rv_out_dev, void *work, void *stream);
int hpcla_bicg_s_f64(const double *rho_dev, const double *rv_dev, const double *r, const double *v, const double *dinv,
                     double *s, double *sh, int64_t n, int64_t iter, const int64_t *state_dev, void *stream);
int hpcla_bicg_tts_f64(hpcla_comm_t *comm, const double *t, const double *s, int64_t n, int64_t iter, int64_t *state_dev,
                       double *triple_out_dev, void *work, void *stream);
int hpcla_bicg_xr_f64(hpcla_comm_t *comm, const double *rho_dev, const double *rv_dev, const double *triple_dev,
                      const double *ph, const double *sh, const double *s, const double *t, const double *rhat, double *x,
                      double *r, int64_t n, int64_t iter, int64_t *state_dev, double *pair_out_dev, void *work,
                      void *stream);
int hpcla_bicg_p_f64(const double *rho_new_dev, const double *rho_dev, const double *rv_dev, const double *triple_dev,
                     const double *r, const double *v, const double *dinv, double *p, double *ph, int64_t n, int64_t iter,
                     const int64_t *state_dev, void *stream);
/* Iterations first_iter .. first_iter + iters - 1 enqueued by ONE host call: per iteration v = A*ph and t = A*sh through
 * hpcla_spmv_dist_* (always executed, no dot partials) and the five steps above.  dinv == NULL: ph and sh are not used
 * (p and s are the SpMV's inputs) and may be NULL.  hist_dev: pairs, [2j] = sum r_j^2 (sum s_j^2 for a half-step stop),
 * [2j+1] = rhat.r_j, the rho of iteration j + 1; pair 0 on entry of the first chunk.  scal_dev: 4 doubles (rv, ts, tt, ss).
 * The state lives in the last 32 bytes of work and is set up by the caller.  Everything else as for
 * hpcla_pcg_iterations_*.  Only enqueues. */
int hpcla_bicgstab_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                      const int32_t *colval_split, const int16_t *cols16,
                                      const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows,
                                      int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                      const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, double *x,
                                      double *r, const double *rhat, double *p, double *ph, double *v, double *s,
                                      double *sh, double *t, double *hist_dev, double *scal_dev, void *work,
                                      int64_t first_iter, int iters, void *stream);
int hpcla_bicgstab_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                      const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                      int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                      const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, double *x,
                                      double *r, const double *rhat, double *p, double *ph, double *v, double *s,
                                      double *sh, double *t, double *hist_dev, double *scal_dev, void *work,
                                      int64_t first_iter, int iters, void *stream);
/* ---- LSQR for a rectangular A (m x n): min |A x - b|^2 + damp^2 |x|^2 by Golub-Kahan bidiagonalisation on A and its
 * materialised transpose At (no reference counterpart: A \ b goes through MUMPS on the host and needs a square A; a caller of
 * the reference's operators composes the method from A*v, src/sparse.jl:2096-2128, transpose(A)*u, src/sparse.jl:2136-2142,
 * norm, src/vectors.jl:758-780, and the broadcasts, src/vectors.jl:1203-1226: two normalisation passes and four host
 * read-backs per iteration).  No vector is normalised in memory: uh and vh are kept unnormalised next to their norms beta
 * and alpha, and the scalings ride in the passes below.
 * The state is the CG solver's (done_iter, status, thr, ntol2) with one more status and the fourth word in use:
 *   3 least squares (|Abar' rbar|^2 <= ntol2 * anorm2 * |rbar|^2 at done_iter); thr = max(rtol |b|, atol)^2, ntol2 = ntol^2.
 * scal_dev: 24 doubles.  Slots: 0 alpha, 1 beta, 2 uu (= uh.uh, all-reduced), 3 vv (= vh.vh, all-reduced), 4 phibar,
 * 5 rhobar, 6 res2, 7 anorm2, 8 t1, 9 t2, 10 rho, 11 c, 12 s, 13 theta, 14 phi, 15 rn2, 16 arn, 17 damp (the caller's, never
 * written), 18 .. 23 reserved.  Before the first iteration: alpha, beta, phibar = beta, rhobar = alpha, damp; the rest 0.
 * Iteration `iter` is 1-based over the whole solve; every entry is a no-op writing no byte once status != 0 (lsqr_xw runs
 * once more, x only, when status is 1 or 3 and done_iter == iter).  Each sum is all-reduced once (comm != NULL):
 *   lsqr_u   (scale, axpy, norm)  uh = tu / alpha - (alpha / beta) * uh;  uu = uh.uh.  No gate.
 *   lsqr_v   (scale, axpy, norm)  beta' = sqrt(uu);  vh = tv / beta' - (beta' / alpha) * vh;  vv = vh.vh.  Gate U: uu == 0:
 *                                 vh is not written and vv = 0.  Then, pair_out_dev != NULL, the step by one thread, behind
 *                                 the all-reduce, with alpha' = sqrt(vv):
 *                                   anorm2 += (alpha^2 + beta'^2) + damp^2
 *                                   rhobar1 = sqrt(rhobar^2 + damp^2);  psi = (damp / rhobar1) * phibar
 *                                   phibar = (rhobar / rhobar1) * phibar;  res2 += psi^2
 *                                   rho = sqrt(rhobar1^2 + beta'^2);  c = rhobar1 / rho;  s = beta' / rho
 *                                   theta = s * alpha';  rhobar = -c * alpha';  phi = c * phibar;  phibar = s * phibar
 *                                   t1 = phi / rho;  t2 = theta / rho;  rn2 = phibar^2 + res2;  arn = alpha' * |s * phi|
 *                                   pair_out_dev = (rn2, arn^2);  alpha = alpha';  beta = beta'
 *                                 and its gates, in this order:
 *                                   rn2 or arn not finite:              status = 2, done_iter = iter - 1
 *                                   rn2 <= thr:                         status = 1, done_iter = iter
 *                                   arn^2 <= (ntol2 * anorm2) * rn2:    status = 3, done_iter = iter
 *                                 pair_out_dev == NULL: no step, no gate (the setup's vh = tv / beta from vh = 0, alpha = 1).
 *   lsqr_xw  (two axpys, scale)   x = x + t1 * w;  w = vh / alpha - t2 * w (alpha is the step's alpha').  In the iteration
 *                                 that stopped only x = x + t1 * w.  After a breakdown x keeps its value of iter - 1.
 * Separate divide, multiply and subtract, in the order written.  tu and tv (HPCLA_CG_NT bit 2) and x (bit 0) go
 * non-temporally.  work: hpcla_lsqr_work_bytes() bytes -- one array of partials, then the 32 bytes the iterations entry
 * uses as the state.  Vectors 16-byte aligned. */
int64_t hpcla_lsqr_work_bytes(void);
int hpcla_lsqr_u_f64(hpcla_comm_t *comm, double *scal_dev, const double *tu, double *uh, int64_t n, int64_t iter,
                     const int64_t *state_dev, void *work, void *stream);
int hpcla_lsqr_v_f64(hpcla_comm_t *comm, double *scal_dev, const double *tv, double *vh, int64_t n, int64_t iter,
                     int64_t *state_dev, double *pair_out_dev, void *work, void *stream);
int hpcla_lsqr_xw_f64(const double *scal_dev, const double *vh, double *x, double *w, int64_t n, int64_t iter,
                      const int64_t *state_dev, void *stream);
/* Iterations first_iter .. first_iter + iters - 1 enqueued by ONE host call: per iteration tu = A*vh on A's plan, lsqr_u,
 * tv = At*uh on At's plan (both through hpcla_spmv_dist_*, always executed), lsqr_v with its step, lsqr_xw.  The plan and CSR
 * arguments of hpcla_bicgstab_iterations_* come twice: for A (nrows = m local rows; its x operand has nrows_t entries) and,
 * suffixed _t, for At (nrows_t = n local rows).  uh, tu: nrows doubles; x, vh, w, tv: nrows_t doubles.  hist_dev: pairs,
 * [2j] = |rbar_j|^2 and [2j+1] = |Abar' rbar_j|^2 of the recurrences (global on every rank, not all-reduced); pair 0 is the
 * caller's.  The state lives in the last 32 bytes of work and is set up by the caller.  Only enqueues. */
int hpcla_lsqr_iterations_f64_i32(hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int32_t *rowptr,
                                  const int32_t *colval_split, const int16_t *cols16, const hpcla_block_patterns_t *patterns,
                                  const double *nzval, int64_t nrows, int64_t nnz, int index_base,
                                  const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                                  int64_t n_boundary, hpcla_halo_plan_t *plan_t, const int32_t *rowptr_t,
                                  const int32_t *colval_split_t, const int16_t *cols16_t,
                                  const hpcla_block_patterns_t *patterns_t, const double *nzval_t, int64_t nrows_t,
                                  int64_t nnz_t, int index_base_t, const int32_t *interior_blocks_t, int64_t n_interior_t,
                                  const int32_t *boundary_blocks_t, int64_t n_boundary_t, double *x, double *uh, double *vh,
                                  double *w, double *tu, double *tv, double *hist_dev, double *scal_dev, void *work,
                                  int64_t first_iter, int iters, void *stream);
int hpcla_lsqr_iterations_f64_i64(hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int64_t *rowptr,
                                  const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz, int index_base,
                                  const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                                  int64_t n_boundary, hpcla_halo_plan_t *plan_t, const int64_t *rowptr_t,
                                  const int64_t *colval_split_t, const double *nzval_t, int64_t nrows_t, int64_t nnz_t,
                                  int index_base_t, const int32_t *interior_blocks_t, int64_t n_interior_t,
                                  const int32_t *boundary_blocks_t, int64_t n_boundary_t, double *x, double *uh, double *vh,
                                  double *w, double *tu, double *tv, double *hist_dev, double *scal_dev, void *work,
                                  int64_t first_iter, int iters, void *stream);
/* ---- MINRES for a symmetric, possibly indefinite A: A x = b by Paige and Saunders' Lanczos recurrence with a positive
 * definite diagonal preconditioner M = dinv .* or the identity (the reference serves this class with ldlt(A) \ b through MUMPS
 * on the host, src/mumps_factorization.jl:247-259; a caller of its operators composes the method from A*v,
 * src/sparse.jl:2096-2128, dot, src/vectors.jl:798-812, and the broadcasts, src/vectors.jl:1203-1226: about ten launches and
 * three host read-backs per iteration).  No vector is normalised in memory: the Lanczos vectors r1, r2 are kept unnormalised
 * next to their M-norms oldb and beta, y = M r2 is the SpMV's operand (r2 itself when dinv == NULL), v = y / beta is never
 * stored.
 * The state is the CG solver's (done_iter, status, thr, reserved); thr = max(rtol sqrt(b.M b), atol)^2: with dinv the stop rule
 * is in the M norm, sqrt(r.M r).
 * scal_dev: 16 doubles.  Slots: 0 beta, 1 oldb, 2 yt (= y.t, the SpMV's, all-reduced), 3 bb (= rn.yn, all-reduced), 4 alfa,
 * 5 cs, 6 sn, 7 dbar, 8 epsln, 9 oldeps, 10 delta, 11 gbar, 12 gamma, 13 phi, 14 phibar, 15 reserved.  Before the first
 * iteration: beta = phibar = sqrt(r0.M r0), cs = -1; the rest 0.
 * Iteration `iter` is 1-based over the whole solve; every entry is a no-op writing no byte once status != 0 (minres_xw runs
 * once more when status == 1 and done_iter == iter).  The sum is all-reduced once (comm != NULL):
 *   minres_r  (two scales, two axpys, [a product,] dot)
 *                                 alfa = yt / (beta * beta);  rn = (t / beta - (alfa / beta) * r2) - (beta / oldb) * r1, written
 *                                 over r1 (iter == 1: no r1 term, r1 is only written);  dinv != NULL: yn = dinv .* rn;
 *                                 bb = rn.yn (rn.rn without dinv; yn may be NULL then).  32 bytes per row, 48 with dinv.  Then,
 *                                 pair_out_dev != NULL, the step by one thread, behind the all-reduce:
 *                                   gate N  !(bb >= 0), or bb or alfa not finite:  status = 2, done_iter = iter - 1
 *                                   beta' = sqrt(bb);  oldeps = epsln;  delta = cs * dbar + sn * alfa
 *                                   gbar = sn * dbar - cs * alfa;  epsln = sn * beta';  dbar = (-cs) * beta'
 *                                   gamma = sqrt(gbar * gbar + beta' * beta')
 *                                   gate G  !(gamma > 0):                          status = 2, done_iter = iter - 1
 *                                   cs = gbar / gamma;  sn = beta' / gamma;  phi = cs * phibar;  phibar = sn * phibar
 *                                   pair_out_dev = (phibar * phibar, bb);  oldb = beta;  beta = beta'
 *                                   gate C  phibar * phibar <= thr:                status = 1, done_iter = iter
 *                                 A gate that reports a breakdown writes no scalar.  pair_out_dev == NULL: no step, no gate
 *                                 (the setup's r2 = t, y = dinv .* r2, bb = r2.y from beta = 1, yt = 0 and r2 = 0).
 *   minres_xw (a scale, three axpys)  w = ((y / oldb - oldeps * w1) - delta * w2) / gamma, written over w1;  x = x + phi * w.
 *                                 y is the operand of this iteration's SpMV and oldb, after the step, its norm.  48 bytes per
 *                                 row.  After a breakdown x keeps its value of iter - 1.
 * Separate divide, multiply, add, subtract and square root, in the order written.  t (HPCLA_CG_NT bit 2) and x (bit 0) go
 * non-temporally.  work: hpcla_minres_work_bytes() bytes -- one array of partials, then the 32 bytes the iterations entry
 * uses as the state.  Vectors 16-byte aligned; a written vector aliases no other. */
int64_t hpcla_minres_work_bytes(void);
int hpcla_minres_r_f64(hpcla_comm_t *comm, double *scal_dev, const double *t, const double *r2, const double *dinv, double *r1,
                       double *yn, int64_t n, int64_t iter, int64_t *state_dev, double *pair_out_dev, void *work,
                       void *stream);
int hpcla_minres_xw_f64(const double *scal_dev, const double *y, const double *w2, double *w1, double *x, int64_t n,
                        int64_t iter, const int64_t *state_dev, void *stream);
/* Iterations first_iter .. first_iter + iters - 1 enqueued by ONE host call: per iteration t = A*y with yt = y.t into slot 2
 * (hpcla_spmv_dist_dot_*, always executed), minres_r with its step, minres_xw.  Two buffers each of r, w and (dinv != NULL) y
 * rotate by the parity of the iteration: iteration j reads r2, y and w2 from the buffers (j - 1) & 1 (0: _a, 1: _b) and
 * overwrites the buffers j & 1; before iteration 1 r_a = r0, y_a = dinv .* r0, w_a = w_b = 0.  dinv == NULL: y_a and y_b are
 * not used and may be NULL.  hist_dev: pairs, [2j] = phibar_j^2 (the squared residual norm of the recurrence, in the M norm)
 * and [2j+1] = beta_{j+1}^2 (global on every rank, not all-reduced); pair 0 is the caller's.  dot_work: the byte count of
 * hpcla_spmv_dot_work_bytes.  The state lives in the last 32 bytes of work and is set up by the caller.  Everything else as
 * for hpcla_pcg_iterations_*.  Only enqueues. */
int hpcla_minres_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                    const int32_t *colval_split, const int16_t *cols16, const hpcla_block_patterns_t *patterns,
                                    const double *nzval, int64_t nrows, int64_t nnz, int index_base,
                                    const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                                    int64_t n_boundary, const double *dinv, double *x, double *r_a, double *r_b, double *y_a,
                                    double *y_b, double *w_a, double *w_b, double *t, double *hist_dev, double *scal_dev,
                                    void *dot_work, void *work, int64_t first_iter, int iters, void *stream);
int hpcla_minres_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                    const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz, int index_base,
                                    const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                                    int64_t n_boundary, const double *dinv, double *x, double *r_a, double *r_b, double *y_a,
                                    double *y_b, double *w_a, double *w_b, double *t, double *hist_dev, double *scal_dev,
                                    void *dot_work, void *work, int64_t first_iter, int iters, void *stream);
/* ---- Restarted GMRES(m) for nonsymmetric A: gated steps of right-preconditioned GMRES with twice-applied classical
 * Gram-Schmidt, K = identity or dinv .* (no reference counterpart; a caller of the reference's operators composes the method
 * from A*p, src/sparse.jl:2096-2128, dot, src/vectors.jl:798-812, and the broadcasts, src/vectors.jl:1203-1226: 2c dots, 2c
 * axpys and 2c + 1 host read-backs in the step that orthogonalises against c basis columns).
 * The basis is V: restart + 1 columns of n doubles at pitch ldv >= n, ldv even, so that every column is 16-byte aligned.
 * The state is the CG solver's (done_iter, status, thr, reserved) with one more status:
 *   3 converged at a restart (the true residual's sum of squares <= thr at done_iter); callers report "converged".
 * The small arrays of a solve live in ONE buffer of hpcla_gmres_small_offset(restart, 10) doubles; the offset of each is
 * hpcla_gmres_small_offset(restart, which), which = 0 .. 9:  R (restart x restart, column j at R + j*restart), c, s (the
 * rotations), g (restart + 1), h1, h2 (the two passes' coefficients), col (restart + 1, scratch), y, nn (w.w), hn (the
 * divisor of hpcla_gmres_next_f64: sqrt(nn), or beta at a restart).  Both return -1 for a restart outside 1..64.
 * Step `iter` is 1-based over the whole solve; every entry is a no-op writing no byte once status != 0 (solve and xupdate
 * are ungated when state_dev == NULL).  Each reduction is all-reduced (comm != NULL) before it is used:
 *   gmres_dots      h_out_dev[i] = V_i . w, i < ncols, all-reduced in slices of at most 8 sums.  A column's sum has the
 *                   same bits whatever ncols is.  work: hpcla_gmres_work_bytes(restart) bytes with restart >= ncols.
 *   gmres_update    w = ((w - h_dev[0]*V_0) - h_dev[1]*V_1) - ... in one pass.  small_dev == NULL: nothing else (restart,
 *                   hist_k_dev and work are not used).  Else also nn = w.w, one all-reduce, and the small step of column
 *                   j = ncols - 1:  col[i] = h1[i] + h2[i], col[ncols] = hn = sqrt(nn);  the stored rotations i < j
 *                   (t = c_i*col[i] + s_i*col[i+1];  col[i+1] = (-s_i)*col[i] + c_i*col[i+1];  col[i] = t);
 *                   d = sqrt(col[j]^2 + col[j+1]^2).  Gate D: !(d > 0), NaN included: status = 2, done_iter = iter - 1,
 *                   nothing of column j stored.  Else c_j = col[j]/d, s_j = col[j+1]/d, R[0..j, j] = col[0..j-1], d;
 *                   g[j+1] = (-s_j)*g[j], g[j] = c_j*g[j];  *hist_k_dev = g[j+1]^2.  Gate C: that <= thr: status = 1,
 *                   done_iter = iter.
 *   gmres_next      v_next = w / *hn_dev (a division);  z = dinv .* v_next when dinv != NULL (z may be NULL otherwise).
 *   gmres_solve     y = R^-1 g over ncols columns by back substitution.
 *   gmres_xupdate   u = y_dev[0]*V_0;  u = u + y_dev[i]*V_i ascending;  x = x + u, or x + dinv .* u.
 *   gmres_residual  w = b - w (w holds A*x);  rr = w.w, one all-reduce.  Gate R at iter >= 0: rr <= thr: status = 3,
 *                   done_iter = iter, *hist_k_dev = rr.  Else g = (sqrt(rr), 0, ...), hn = sqrt(rr), and *hist_k_dev = rr
 *                   when iter == 0.
 *   gmres_finish    the host's end of an open cycle, ungated: gmres_solve and gmres_xupdate over ncols columns; ncols == 0
 *                   does nothing.
 * Separate multiply, add, subtract, divide and sqrt, in the order written.  work: hpcla_gmres_work_bytes(restart) bytes --
 * one array of partials per column (whole tiles of 8), then the 32 bytes the iterations entry uses as the state.  Vectors
 * 16-byte aligned. */
int64_t hpcla_gmres_work_bytes(int restart);
int64_t hpcla_gmres_small_offset(int restart, int which);
int hpcla_gmres_dots_f64(hpcla_comm_t *comm, const double *V, int64_t ldv, int ncols, const double *w, int64_t n,
                         const int64_t *state_dev, double *h_out_dev, void *work, void *stream);
int hpcla_gmres_update_f64(hpcla_comm_t *comm, const double *V, int64_t ldv, int ncols, const double *h_dev, double *w,
                           int64_t n, int64_t iter, int restart, double *small_dev, double *hist_k_dev, int64_t *state_dev,
                           void *work, void *stream);
int hpcla_gmres_next_f64(const double *w, const double *hn_dev, const double *dinv, double *v_next, double *z, int64_t n,
                         const int64_t *state_dev, void *stream);
int hpcla_gmres_solve_f64(int ncols, int restart, double *small_dev, const int64_t *state_dev, void *stream);
int hpcla_gmres_xupdate_f64(const double *V, int64_t ldv, int ncols, const double *y_dev, const double *dinv, double *x,
                            int64_t n, const int64_t *state_dev, void *stream);
int hpcla_gmres_residual_f64(hpcla_comm_t *comm, const double *b, double *w, int64_t n, int64_t iter, int restart,
                             double *small_dev, double *hist_k_dev, int64_t *state_dev, void *work, void *stream);
int hpcla_gmres_finish_f64(const double *V, int64_t ldv, int ncols, int restart, double *small_dev, const double *dinv,
                           double *x, int64_t n, void *stream);
/* Steps first_iter .. first_iter + iters - 1 enqueued by ONE host call: per step w = A*z through hpcla_spmv_dist_* (always
 * executed; z is basis column j = (k-1) mod restart when dinv == NULL, and z may then be NULL), dots, update, dots, update
 * with the small step, and gmres_next while j + 1 < restart; at j + 1 == restart, all gated, gmres_solve, gmres_xupdate and
 * the restart (below) at iteration k.  hist_dev: pairs as for the other solvers, [2k] = the Givens estimate g[j+1]^2 of
 * sum r_k^2 (the true one at k = 0 and at a gate R stop), [2k+1] not used.  The state lives in the last 32 bytes of work and
 * is set up by the caller.  Everything else as for hpcla_bicgstab_iterations_*.  Only enqueues. */
int hpcla_gmres_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                   const int32_t *colval_split, const int16_t *cols16,
                                   const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows, int64_t nnz,
                                   int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                   const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, const double *b,
                                   double *x, double *V, int64_t ldv, double *w, double *z, double *small_dev,
                                   double *hist_dev, void *work, int restart, int64_t first_iter, int iters, void *stream);
int hpcla_gmres_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                   const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                   int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                   const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, const double *b,
                                   double *x, double *V, int64_t ldv, double *w, double *z, double *small_dev,
                                   double *hist_dev, void *work, int restart, int64_t first_iter, int iters, void *stream);
/* The start of a cycle at iteration iter >= 0: w = A*x, gmres_residual, then V_0 = w / beta [z = dinv .* V_0] into the
 * first column of V.  The solver's setup from a given x0 (iter = 0) and the end of every full cycle. */
int hpcla_gmres_restart_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                const int32_t *colval_split, const int16_t *cols16, const hpcla_block_patterns_t *patterns,
                                const double *nzval, int64_t nrows, int64_t nnz, int index_base,
                                const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                                int64_t n_boundary, const double *dinv, const double *b, const double *x, double *V,
                                int64_t ldv, double *w, double *z, double *small_dev, double *hist_dev, void *work,
                                int restart, int64_t iter, void *stream);
int hpcla_gmres_restart_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz, int index_base,
                                const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                                int64_t n_boundary, const double *dinv, const double *b, const double *x, double *V,
                                int64_t ldv, double *w, double *z, double *small_dev, double *hist_dev, void *work,
                                int restart, int64_t iter, void *stream);
/* ---- Extreme eigenpairs of a symmetric A: thick-restart Lanczos (Wu and Simon; Krylov-Schur for symmetric A) with full
 * reorthogonalisation by twice-applied classical Gram-Schmidt (no reference counterpart: the reference has no eigensolver; a
 * caller of its operators composes Lanczos from A*p, src/sparse.jl:2096-2128, dot, src/vectors.jl:798-812, and the broadcasts,
 * src/vectors.jl:1203-1226: 2c dots, 2c axpys and 2c + 1 host read-backs in the step that orthogonalises against c columns,
 * and the restart V[:, 0:p] = V[:, 0:m] * S as a dense product plus a copy back).
 * The basis is the GMRES one: ncv + 1 columns of n doubles at an even pitch ldv >= n.  The step reuses gmres_dots, the first
 * pass of gmres_update and gmres_next as they are; the state is the CG solver's (done_iter, status, thr [not used], reserved)
 * with status 2 = breakdown and one more:
 *   4 invariant: the new vector is exactly zero at done_iter, the Krylov space is invariant and its Ritz pairs are exact.
 * The small arrays of a solve live in ONE buffer of hpcla_eigsh_small_offset(ncv, 6) doubles; the offset of each is
 * hpcla_eigsh_small_offset(ncv, which), which = 0 .. 5:  T (ncv x ncv, column j at T + j*ncv: the projected matrix's upper
 * triangle as the device computed it), beta (ncv), h1, h2 (the two passes' coefficients), nn (w.w), hn (the divisor of
 * hpcla_gmres_next_f64).  -1 for ncv outside 1..64.  Scratch and state: hpcla_gmres_work_bytes(ncv) bytes.
 *   eigsh_update    the second pass of column j = ncols - 1 at step iter (1-based over the solve): w = ((w - h_dev[0]*V_0) -
 *                   h_dev[1]*V_1) - ..., nn = w.w, one all-reduce (comm != NULL), then by one thread:
 *                     gate N  nn != nn:  status = 2, done_iter = iter - 1, nothing of column j is stored
 *                     T[i, j] = h1[i] + h2[i] for i <= j;  beta[j] = hn = sqrt(nn)
 *                     gate I  nn == 0:   status = 4, done_iter = iter (column j is stored)
 *                   Once status != 0 it writes no byte with comm == NULL; with a communicator the all-reduce between the two
 *                   gated launches still runs and rewrites nn (scratch: nothing reads it behind a stop), and nothing else.
 *   eigsh_rotate    the restart, one pass over the basis (csrc/eigsh.hip).  S_dev: m x p, column j at S_dev + j*m.  Row r:
 *                   acc = V[r,0]*S[0,j];  acc = acc + V[r,i]*S[i,j], i ascending, separately rounded.  out == NULL: in place,
 *                   V[:, 0:p] = V[:, 0:m] * S (every lane loads its whole row before it stores), and column p receives old
 *                   column m when move_last != 0; columns beyond, and the pad of an odd n, are untouched.  out != NULL
 *                   (move_last must be 0): V is only read and the n x p product goes to out[r*out_row_stride +
 *                   j*out_col_stride].  1 <= p <= m <= 64; V 16-byte aligned.  8 (m + p) + 16 bytes per row in place. */
int64_t hpcla_eigsh_small_offset(int ncv, int which);
int hpcla_eigsh_update_f64(hpcla_comm_t *comm, const double *V, int64_t ldv, int ncols, const double *h_dev, double *w,
                           int64_t n, int64_t iter, int ncv, double *small_dev, int64_t *state_dev, void *work, void *stream);
int hpcla_eigsh_rotate_f64(double *V, int64_t ldv, int m, int p, const double *S_dev, int move_last, double *out,
                           int64_t out_row_stride, int64_t out_col_stride, int64_t n, void *stream);
/* Columns first_col .. first_col + count - 1 of a cycle (steps first_iter .. of the solve) enqueued by ONE host call: per
 * column j, w = A*V_j through hpcla_spmv_dist_* (always executed), gmres_dots into h1, gmres_update (first pass), gmres_dots
 * into h2, eigsh_update, and gmres_next into column j + 1 (also at j + 1 == ncv).  The state lives in the last 32 bytes of
 * work and is set up by the caller.  Everything else as for hpcla_gmres_iterations_*.  Only enqueues. */
int hpcla_eigsh_steps_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr, const int32_t *colval_split,
                              const int16_t *cols16, const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows,
                              int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
                              const int32_t *boundary_blocks, int64_t n_boundary, double *V, int64_t ldv, double *w,
                              double *small_dev, void *work, int ncv, int first_col, int count, int64_t first_iter,
                              void *stream);
int hpcla_eigsh_steps_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr, const int64_t *colval_split,
                              const double *nzval, int64_t nrows, int64_t nnz, int index_base, const int32_t *interior_blocks,
                              int64_t n_interior, const int32_t *boundary_blocks, int64_t n_boundary, double *V, int64_t ldv,
                              double *w, double *small_dev, void *work, int ncv, int first_col, int count, int64_t first_iter,
                              void *stream);
/* ---- The largest singular triplets of a rectangular A: thick-restart Golub-Kahan-Lanczos bidiagonalisation (Baglama and
 * Reichel; SLEPc's TRLBD) with full two-sided reorthogonalisation by twice-applied classical Gram-Schmidt (no reference
 * counterpart: the reference has no SVD, its svd would be a dense LAPACK call; a caller of its operators composes the method
 * from A*v, src/sparse.jl:2096-2128, transpose(A)*u, src/sparse.jl:2136-2142, dot, src/vectors.jl:798-812, and the broadcasts,
 * src/vectors.jl:1203-1226: 4c dots, 4c axpys and 4c + 2 host read-backs in the step that orthogonalises against c columns on
 * each side, and the restart as two dense products plus their copies back).
 * Two bases of the GMRES kind: U, ncv columns of nrows doubles, and V, ncv + 1 columns of nrows_t doubles, each at an even
 * pitch of its own and 16-byte aligned.  Each half of a step reuses gmres_dots, the first pass of gmres_update and gmres_next as
 * they are; the restart is two launches of hpcla_eigsh_rotate_f64; the state is the eigensolver's (done_iter, status, not used,
 * reserved) with status 2 = breakdown and 4 = invariant.
 * The small arrays of a solve live in ONE buffer of hpcla_svds_small_offset(ncv, 9) doubles; the offset of each is
 * hpcla_svds_small_offset(ncv, which), which = 0 .. 8:  B (ncv x ncv, column j at B + j*ncv: the projected matrix's upper
 * triangle as the device computed it, alpha_j on its diagonal; the strict lower triangle is never written), beta (ncv), g1, g2
 * (the left half's two passes' coefficients), h1, h2 (the right half's), aa (u.u), bb (v.v), dv (the divisor of
 * hpcla_gmres_next_f64).  -1 for ncv outside 1..64.  Scratch and state: hpcla_gmres_work_bytes(ncv) bytes.
 *   svds_update     the second pass of one half of column j at step iter (1-based over the solve): w = ((w - h_dev[0]*W_0) -
 *                   h_dev[1]*W_1) - ..., nn = w.w, one all-reduce (comm != NULL), then by one thread the small step of that side.
 *                   side 0 (left: W = U, ncols = j, 0 <= ncols <= ncv - 1; ncols == 0 is the norm and the small step alone, W
 *                   and h_dev may then be NULL), nn goes to aa:
 *                     gate N   aa != aa:  status = 2, done_iter = iter - 1, nothing of column j is stored
 *                     B[i, j] = g1[i] + g2[i] for i < j;  B[j, j] = dv = sqrt(aa)
 *                     gate Z   aa == 0:   status = 4, done_iter = iter - 1 (j triplets are finished; column j of B is stored)
 *                   side 1 (right: W = V, ncols = j + 1, 1 <= ncols <= ncv), nn goes to bb:
 *                     gate N'  bb != bb:  status = 2, done_iter = iter - 1, beta[j] is not stored
 *                     beta[j] = dv = sqrt(bb)
 *                     gate Z'  bb == 0:   status = 4, done_iter = iter (j + 1 triplets are finished; beta[j] = 0 is stored)
 *                   With c = done_iter - (steps before the cycle) + p finished columns the gate was Z' when c > p and
 *                   beta[c - 1] == 0, else Z.  The sum's order is hpcla_dot_f64's and does not depend on ncols.
 *                   Once status != 0 it writes no byte with comm == NULL; with a communicator the all-reduce between the two
 *                   gated launches still runs and rewrites aa or bb (scratch: nothing reads it behind a stop), and nothing else. */
int64_t hpcla_svds_small_offset(int ncv, int which);
int hpcla_svds_update_f64(hpcla_comm_t *comm, const double *W, int64_t ldw, int ncols, const double *h_dev, double *w, int64_t n,
                          int64_t iter, int ncv, int side, double *small_dev, int64_t *state_dev, void *work, void *stream);
/* Columns first_col .. first_col + count - 1 of a cycle (steps first_iter .. of the solve) enqueued by ONE host call.  The two
 * matrix blocks are A's and its materialised transpose's, as hpcla_lsqr_iterations_* takes them.  Per column j: u = A*V_j
 * (always executed), over U's j columns (nothing at j == 0) gmres_dots into g1, gmres_update (first pass), gmres_dots into g2,
 * then svds_update (side 0) and gmres_next into U_j; v = At*U_j (always executed), over V's j + 1 columns gmres_dots into h1,
 * gmres_update, gmres_dots into h2, svds_update (side 1) and gmres_next into V_{j+1} (also at j + 1 == ncv).  The state lives in
 * the last 32 bytes of work and is set up by the caller.  Only enqueues. */
int hpcla_svds_steps_f64_i32(hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int32_t *rowptr, const int32_t *colval_split,
                             const int16_t *cols16, const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows,
                             int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
                             const int32_t *boundary_blocks, int64_t n_boundary, hpcla_halo_plan_t *plan_t,
                             const int32_t *rowptr_t, const int32_t *colval_split_t, const int16_t *cols16_t,
                             const hpcla_block_patterns_t *patterns_t, const double *nzval_t, int64_t nrows_t, int64_t nnz_t,
                             int index_base_t, const int32_t *interior_blocks_t, int64_t n_interior_t,
                             const int32_t *boundary_blocks_t, int64_t n_boundary_t, double *U, int64_t ldu, double *V,
                             int64_t ldv, double *u, double *v, double *small_dev, void *work, int ncv, int first_col, int count,
                             int64_t first_iter, void *stream);
int hpcla_svds_steps_f64_i64(hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int64_t *rowptr, const int64_t *colval_split,
                             const double *nzval, int64_t nrows, int64_t nnz, int index_base, const int32_t *interior_blocks,
                             int64_t n_interior, const int32_t *boundary_blocks, int64_t n_boundary, hpcla_halo_plan_t *plan_t,
                             const int64_t *rowptr_t, const int64_t *colval_split_t, const double *nzval_t, int64_t nrows_t,
                             int64_t nnz_t, int index_base_t, const int32_t *interior_blocks_t, int64_t n_interior_t,
                             const int32_t *boundary_blocks_t, int64_t n_boundary_t, double *U, int64_t ldu, double *V,
                             int64_t ldv, double *u, double *v, double *small_dev, void *work, int ncv, int first_col, int count,
                             int64_t first_iter, void *stream);
/* ---- the block eigensolver (hp.lobpcg, csrc/lobpcg.hip): LOBPCG with B = I for the k <= 16 smallest or largest eigenpairs of
 * a symmetric A.  The host enqueues, per iteration: lobpcg_residual, the SpMM A*W (hpcla_spmm_*), ONE hpcla_gram_f64 of
 * S = [X W P] against [S | AS], reads the residual sums and the Gram matrices back once, solves the whitened Rayleigh-Ritz
 * problem in numpy, uploads (theta, C) and runs lobpcg_combine.  Every block is row-major with a pitch (in doubles) of its own,
 * so the blocks may be column ranges of one wider buffer; every array is 8-byte aligned, and where all the pitches of a call
 * are even and its bases 16-byte aligned the accesses are 16 bytes per lane.  1 <= k <= 16.
 *   lobpcg_residual  per element, separately rounded:  t = theta_dev[j] * X[r,j];  d = AX[r,j] - t;  W[r,j] = minv[r] * d
 *                    (minv == NULL: W[r,j] = d).  W2 != NULL: the same values go to a second block on the pitch ldw2 (the
 *                    SpMM's operand on spmm_pitch; padding columns of any block are neither read nor written).
 *                    rn2_dev[j] = sum_r d[r,j]^2 (the residual before minv): per-workgroup partials over chunks of hpcla_lobpcg_chunk_rows(n) rows, then
 *                    one workgroup adds the chunks in 16 phases of ascending chunks and the phases ascending -- an order that
 *                    depends on (n, k) only, so the same inputs give the same bits on every call -- then one all-reduce of the
 *                    k sums (comm != NULL).  n == 0: the sums are zero and the rank still reduces; no pointer but rn2_dev is
 *                    looked at.  work: hpcla_lobpcg_work_bytes(n, k) device bytes.  Bytes per row: read 8 (2k + 1 with minv),
 *                    write 8k (16k with W2).
 *   lobpcg_combine   [X | P] <- S C in place, one pass.  S holds [X W P] in columns 0..3k-1 of which the first k + c_rest are
 *                    read, c_rest in {0, k, 2k}; C_dev is (k + c_rest) x k, row i at C_dev + 16 i (the 16 - k doubles behind a
 *                    row are read and ignored).  Per row r and column j, products and sums separately rounded:
 *                      px = 0;  px = px + S[r,i] * C[i,j], i = 0 .. k-1 ascending
 *                      pp = 0;  pp = pp + S[r,i] * C[i,j], i = k .. k + c_rest - 1 ascending
 *                      X'[r,j] = px + pp (columns 0..k-1);  P'[r,j] = pp (columns 2k..3k-1; not written with c_rest = 0)
 *                    and the same for AS != NULL (its own pitch).  Columns k..2k-1 (W) and everything behind 3k keep their
 *                    bits.  In place is safe because a row belongs to one workgroup, which holds the row in LDS before a
 *                    barrier and stores only behind it.  Pitches: at least k, and at least 3k with c_rest > 0.  Returns at
 *                    n == 0.  Bytes per row: read 16 (k + c_rest), write 32k (16k with c_rest = 0); half of both without AS. */
int64_t hpcla_lobpcg_chunk_rows(int64_t n);
int64_t hpcla_lobpcg_work_bytes(int64_t n, int k);
int hpcla_lobpcg_residual_f64(hpcla_comm_t *comm, const double *X, int64_t ldx, const double *AX, int64_t ldax,
                              const double *theta_dev, const double *minv, double *W, int64_t ldw, double *W2, int64_t ldw2,
                              int64_t n, int k, double *rn2_dev, void *work, void *stream);
int hpcla_lobpcg_combine_f64(double *S, int64_t lds, double *AS, int64_t ldas, const double *C_dev, int k, int c_rest,
                             int64_t n, void *stream);
/* ---- the block eigensolver on a pencil (hp.lobpcg with B; csrc/lobpcg.hip): A x = lambda B x, B symmetric positive definite.
 * The reference has no eigensolver, so these entries have no counterpart there either.  The host keeps a third block
 * BS = [BX BW BP] next to S and AS, takes [S'AS | S'BS] from ONE hpcla_gram_f64 of S against [AS | BS], and applies
 * lobpcg_combine a second time to BS (AS == NULL).  Blocks, pitches and alignment as above.  1 <= k <= 16.
 *   lobpcg_residual_gen  per element, separately rounded:  t = theta_dev[j] * BX[r,j];  d = AX[r,j] - t;  w = minv[r] * d
 *                    (minv == NULL: w = d);  W[r,j] = w;  W2 != NULL: W2[r,j] = w (the SpMM's operand on spmm_pitch);
 *                    bdiag != NULL (a diagonal B, given together with BW or not at all): BW[r,j] = bdiag[r] * w, so B W
 *                    needs no product.  Padding columns of any block are neither read nor written.  Three sums per column,
 *                    16 apart:  sums_dev[j] = sum_r d[r,j]^2 (the residual before minv),  sums_dev[16 + j] = sum_r AX[r,j]^2,
 *                    sums_dev[32 + j] = sum_r BX[r,j]^2;  the entries j >= k of a group are not written (with comm != NULL
 *                    they take part in the reduction).  The summation order is lobpcg_residual's -- chunks of
 *                    hpcla_lobpcg_chunk_rows(n) rows, 16 phases of ascending chunks, the phases ascending, a function of
 *                    (n, k) only: the same inputs give the same bits on every call -- then ONE all-reduce of the 48 doubles
 *                    (comm != NULL).  n == 0: the 3k sums are zero and the rank still reduces; no pointer but sums_dev is
 *                    looked at.  work: hpcla_lobpcg_gen_work_bytes(n, k) device bytes.  Bytes per row: read 16k (+8 with
 *                    minv, +8 with bdiag), write 8k per output block (W, W2, BW). */
int64_t hpcla_lobpcg_gen_work_bytes(int64_t n, int k);
int hpcla_lobpcg_residual_gen_f64(hpcla_comm_t *comm, const double *AX, int64_t ldax, const double *BX, int64_t ldbx,
                                  const double *theta_dev, const double *minv, const double *bdiag, double *W, int64_t ldw,
                                  double *W2, int64_t ldw2, double *BW, int64_t ldbw, int64_t n, int k, double *sums_dev,
                                  void *work, void *stream);
/* ---- tall-skinny Householder QR (hp.qr, hp.lstsq; csrc/qr.hip): X = Q R for a row-major n x k block, 1 <= k <= 32, by a
 * communication-avoiding tree of Householder panel factorisations (TSQR).  Reflectors are stored and Q is formed by applying
 * them, so Q'Q = I to rounding whatever the condition number of X is (no Gram matrix, no X inv(R)).
 *   qr_panel_rows    P: the rows of a level-0 panel (one 256-lane workgroup, one lane per row).
 *   qr_fan           F(k) = P / KT, KT = 4, 8, 16 or 32 >= k: the triangles a node of an upper level stacks (0 for a k outside 1..32).
 *   qr_work_bytes    device bytes of `work` for nloc local rows on nranks ranks (tau and a k x k triangle per node of the rank's
 *                    tree, two k x k blocks, and with nranks > 1 the (nranks k) x k stack and its tree); want_q does not raise it.
 *   qr_f64           X: nloc rows on the pitch ldx (>= k), read only.  Q != NULL: nloc rows on the pitch ldq receive the panels'
 *                    reflectors and then, in place, this rank's rows of Q; Q == NULL: R only, nothing of size nloc is written.
 *                    R_dev: k x k on pitch k, upper triangular with exact zeros below and a non-negative diagonal (the signs
 *                    go into Q).  Level 0 factors panels of P rows, level l >= 1 stacks F triangles of the level below, until
 *                    one is left; partial panels are zero-padded, and a column whose sum of squares below the diagonal is
 *                    exactly zero gets tau = 0.  comm with more than one rank: the rank's triangle (zero for nloc == 0) goes
 *                    into its slot of a zeroed (nranks k) x k stack, ONE all-reduce (sum: every slot arrives bit-exact), and
 *                    every rank factors the stack with the same code -- R has the same bits on every rank.  Every sum has an
 *                    order fixed by (nloc, k): the same input gives the same bits on every call.  One launch per level and
 *                    direction; no kernel waits on another workgroup.  Non-finite input propagates into R and Q.  Returns 0
 *                    or a negative status; never aborts.  Bytes per row: 8k read, and with Q 24k more (reflectors written,
 *                    read, Q written). */
int hpcla_qr_panel_rows(void);
int hpcla_qr_fan(int k);
int64_t hpcla_qr_work_bytes(int64_t nloc, int k, int nranks, int want_q);
int hpcla_qr_f64(hpcla_comm_t *comm, const double *X, int64_t ldx, int64_t nloc, int k, double *Q, int64_t ldq, double *R_dev,
                 double *work, void *stream);
int hpcla_divide_f64(const double *x, double a_host, double *y, int64_t n, void *stream);
int hpcla_axpby_f64(double a, const double *x, double b, const double *y, double *z, int64_t n,
                    void *stream);

/* ---- sparse A +/- B value pass: the reference's five index-mapped kernels (_copy_a_only_/
 * _copy_b_only_/_negate_b_only_/_add_both_/_sub_both_kernel!, src/sparse.jl:1258-1303) as ONE pass
 * over the merged pattern: out[i] = a[ia[i]] (+|-) b[ib[i]] where both indices are >= 0, a copy of
 * a[ia[i]] or of (+|-) b[ib[i]] where only one is (never an addition to zero), for i in [0, n).
 * ia/ib (0-based positions in the operands' nzval, -1 = absent) come from the host AdditionPlan
 * (union of the two sparsity patterns, src/sparse.jl:1112-1245).  subtract: 0 = A+B, 1 = A-B. */
int hpcla_merge_combine_f64_i32(double *out, const double *a, const int32_t *ia, const double *b,
                                const int32_t *ib, int64_t n, int subtract, void *stream);
int hpcla_merge_combine_f64_i64(double *out, const double *a, const int64_t *ia, const double *b,
                                const int64_t *ib, int64_t n, int subtract, void *stream);

/* ---- synthetic inputs on the device (bench/tests): the SURVEY section 8d counter-based
 * generator, v[i] = u01(seed, start+i). */
int hpcla_fill_uniform_f64(double *v, int64_t start, int64_t count, uint64_t seed, void *stream);

/* ==== Float32 element type on the hot path (csrc/f32.hip) ======================================================
 * The reference is generic in T; its GPU test configurations are CUDA x {Float32, Float64} and Metal x Float32
 * (test/test_utils.jl:62-80), all through the same _spmv_kernel! (src/sparse.jl:2055-2066: acc = zero(T),
 * acc += nzval[j] * x[colval[j]] in T), the same column loop for A * HPCMatrix (:2391-2413) and the same local
 * dot / nrm2 + scalar all-reduce (src/vectors.jl:758-812).  Float64 is the graded type; these entries give the same
 * path to a Float32 backend: row sums in float, stored order, separate multiply and add (the reference's bits).
 *
 * spmv_csr / spmv_split / spmm_csr / spmm_split: arguments as for the _f64 entries of the same name, with float values,
 * operands and results.  GHOSTS ARE DOUBLES: the halo transports move 8-byte words, so a Float32 exchange widens what it
 * sends (float -> double is exact) and the split kernels narrow the ghost values they gather (exact again); x_ghost_wide
 * / B_ghost_wide are the plan's ordinary ghost segment (hpcla_halo_ghost_ptr).  spmm_split is row-major like its _f64
 * twin; spmm_csr takes either layout for B and C (Julia's column-major Matrix goes in untouched). */
int hpcla_spmv_csr_f32_i32(const int32_t *rowptr, const int32_t *colval, const float *nzval, const float *x, float *y,
                           int64_t nrows, int64_t nnz, int index_base, void *stream);
int hpcla_spmv_csr_f32_i64(const int64_t *rowptr, const int64_t *colval, const float *nzval, const float *x, float *y,
                           int64_t nrows, int64_t nnz, int index_base, void *stream);
int hpcla_spmv_split_f32_i32(const int32_t *rowptr, const int32_t *colval_split, const float *nzval, const float *x_own,
                             const double *x_ghost_wide, int64_t n_own, float *y, int64_t nrows, int64_t nnz,
                             int index_base, const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmv_split_f32_i64(const int64_t *rowptr, const int64_t *colval_split, const float *nzval, const float *x_own,
                             const double *x_ghost_wide, int64_t n_own, float *y, int64_t nrows, int64_t nnz,
                             int index_base, const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmm_csr_f32_i32(const int32_t *rowptr, const int32_t *colval, const float *nzval, const float *B, int64_t ldb,
                           int b_layout, float *C, int64_t ldc, int c_layout, int64_t nrows, int64_t nnz, int k,
                           int index_base, void *stream);
int hpcla_spmm_csr_f32_i64(const int64_t *rowptr, const int64_t *colval, const float *nzval, const float *B, int64_t ldb,
                           int b_layout, float *C, int64_t ldc, int c_layout, int64_t nrows, int64_t nnz, int k,
                           int index_base, void *stream);
int hpcla_spmm_split_f32_i32(const int32_t *rowptr, const int32_t *colval_split, const float *nzval, const float *B_own,
                             int64_t ldb_own, const double *B_ghost_wide, int64_t ldb_ghost, int64_t n_own, float *C,
                             int64_t ldc, int64_t nrows, int64_t nnz, int k, int index_base, const int32_t *block_list,
                             int64_t n_blocks, void *stream);
int hpcla_spmm_split_f32_i64(const int64_t *rowptr, const int64_t *colval_split, const float *nzval, const float *B_own,
                             int64_t ldb_own, const double *B_ghost_wide, int64_t ldb_ghost, int64_t n_own, float *C,
                             int64_t ldc, int64_t nrows, int64_t nnz, int k, int index_base, const int32_t *block_list,
                             int64_t n_blocks, void *stream);
/* column-major own block and result (Julia's Matrix), the plan's row-major ghost segment: hpcla_spmm_split_colmajor_f64_*'s
 * twin for Float32; hpcla_halo_begin_strided_f32 is hpcla_halo_begin_strided_f64's (the staged values are widened) */
int hpcla_spmm_split_colmajor_f32_i32(const int32_t *rowptr, const int32_t *colval_split, const float *nzval,
                                      const float *B_own, int64_t ldb_own, const double *B_ghost_wide, int64_t ldb_ghost,
                                      int64_t n_own, float *C, int64_t ldc, int64_t nrows, int64_t nnz, int k,
                                      int index_base, const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_spmm_split_colmajor_f32_i64(const int64_t *rowptr, const int64_t *colval_split, const float *nzval,
                                      const float *B_own, int64_t ldb_own, const double *B_ghost_wide, int64_t ldb_ghost,
                                      int64_t n_own, float *C, int64_t ldc, int64_t nrows, int64_t nnz, int k,
                                      int index_base, const int32_t *block_list, int64_t n_blocks, void *stream);
int hpcla_halo_begin_strided_f32(hpcla_halo_plan_t *plan, const float *x, int64_t x_rs, int64_t x_cs, double *stage,
                                 void *stream);
/* Distributed y = A*x for Float32 (Base.:*(A, x), src/sparse.jl:2096-2128) in one call: hpcla_halo_begin_f32, the interior
 * blocks (they overlap the exchange), hpcla_halo_end, the boundary blocks with the plan's ghost segment.  Arguments as for
 * hpcla_spmv_dist_f64_* plus `stage` (hpcla_halo_begin_f32).  A plan with attached peer windows must have been created with
 * HPCLA_HALO_SINGLE_BUFFER.  plan == NULL or no neighbours: a plain product over all row blocks. */
int hpcla_spmv_dist_f32_i32(hpcla_halo_plan_t *plan, const int32_t *rowptr, const int32_t *colval_split, const float *nzval,
                            const float *x, int64_t n_own, float *y, int64_t nrows, int64_t nnz, int index_base,
                            const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                            int64_t n_boundary, double *stage, void *stream);
int hpcla_spmv_dist_f32_i64(hpcla_halo_plan_t *plan, const int64_t *rowptr, const int64_t *colval_split, const float *nzval,
                            const float *x, int64_t n_own, float *y, int64_t nrows, int64_t nnz, int index_base,
                            const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                            int64_t n_boundary, double *stage, void *stream);
/* hpcla_halo_begin for a Float32 operand (execute_plan!, src/vectors.jl:394-463): widens x at the plan's send positions
 * into `stage` (doubles, laid out like x: at least (largest send index + 1) * width entries; the caller's, reused from
 * call to call) on `stream`, then posts the ordinary exchange from `stage`.  hpcla_halo_end / hpcla_halo_status /
 * hpcla_halo_ghost_ptr as usual: every transport is the Float64 one. */
int hpcla_halo_begin_f32(hpcla_halo_plan_t *plan, const float *x, double *stage, void *stream);
/* dot / norm pieces (src/vectors.jl:758-812): products and squares are formed and summed in DOUBLE (exact products, two
 * deterministic stages, scalar all-reduce in double); out_dev is a device double, the caller rounds to Float32 once.
 * work: hpcla_reduce_work_bytes().  16-byte aligned operands. */
int hpcla_dot_f32(hpcla_comm_t *comm, const float *x, const float *y, int64_t n, double *out_dev, void *work, void *stream);
int hpcla_nrm2sq_f32(hpcla_comm_t *comm, const float *x, int64_t n, double *out_dev, void *work, void *stream);
int hpcla_asum_f32(hpcla_comm_t *comm, const float *x, int64_t n, double *out_dev, void *work, void *stream);
int hpcla_amax_f32(hpcla_comm_t *comm, const float *x, int64_t n, double *out_dev, void *work, void *stream);
int hpcla_sum_f32(hpcla_comm_t *comm, const float *x, int64_t n, double *out_dev, void *work, void *stream);
int hpcla_maxval_f32(hpcla_comm_t *comm, const float *x, int64_t n, int negate, double *out_dev, void *work, void *stream);
/* z = a*x + b*y, y = a*x, y = x / a in float (src/vectors.jl:868-903, 944-964), separate multiply and add; 16-byte
 * aligned operands. */
/* layout conversion of a Float32 block (hpcla_transpose_f64's twin): column-major Julia Matrix <-> the library's row-major
 * rows, whose ghost rows travel as contiguous k-value pieces in ONE exchange */
int hpcla_transpose_f32(const float *src, int64_t ld_src, int src_layout, float *dst, int64_t ld_dst, int dst_layout,
                        int64_t rows, int64_t cols, void *stream);
int hpcla_axpby_f32(float a, const float *x, float b, const float *y, float *z, int64_t n, void *stream);
int hpcla_scale_f32(float a, const float *x, float *y, int64_t n, void *stream);
int hpcla_divide_f32(const float *x, float a, float *y, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HPCLA_ROCM_H */
