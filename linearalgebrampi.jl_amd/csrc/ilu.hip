// ilu.hip -- the fine-grained ILU(0) preconditioner (hp.ilu0) for the nonsymmetric solvers: Chow-Patel sweeps build the factors,
// truncated Jacobi iterations (Anzt, Chow, Dongarra) stand for the two triangular solves.  No kernel waits on another: every
// launch reads the previous launch's buffers only, so every result is fixed by its inputs.
//
// The block.  Rows and columns of A are partitioned alike (n_own == nrows), so a split column c < n_own IS local row c; columns
// >= n_own are ghosts and are dropped: block-Jacobi ILU.  The owned block is compacted once into a CSR of its own with Int32
// everything (nnz < 2^31): b_rowptr (nrows + 1), b_cols (local columns, ascending within a row whatever A's order), b_rows (the
// row of every entry: the sweep runs one lane per entry), b_diag (the position of a row's diagonal, -1 when none is stored) and
// b_map (the entry's position in A's nzval: new values for the same structure are one gather).  The column-wise view c_ptr /
// c_pos (the entries of column j in ascending row, as positions into the block) is built by the caller with a stable sort.
//
// The factors.  One value array f aligned with the block: l_ij for i > j (unit diagonal not stored), u_ij for i <= j.
//   init     l_ij = a_ij / a_jj, u_ij = a_ij
//   sweep    s = a_ij - sum_{k < min(i, j), (i, k) and (k, j) stored} l_ik * u_kj, ascending k, a two-pointer merge of row i
//            against column j; multiply and subtract separately rounded (-ffp-contract=off).  l_ij = s / u_jj (the previous
//            sweep's u_jj) for i > j, u_ij = s otherwise.  Reads f_old, writes f_new: rows of any length, no scratch, no atomics.
//   pivots   dinv_i = 1 / u_ii; a u_ii that is zero, NaN or infinite lowers the error word.
// Error word (one device word, vector atomic min): (local row << 2) | code of the smallest failing row; all ones = none.  A
// fault in row r can spoil rows >= r only (a sum over k < min(i, j)), and for one row the structural codes are the smaller
// ones, so one read-back after the last sweep names the first cause.  A row without a diagonal contributes NaN, never an
// address.
//
// The application.  z = N_U(N_L(r)), both truncated Neumann series written as Jacobi sweeps on the triangular systems:
//   out_i = (rhs_i - sum_{p in the lower (upper) part of row i} f_p * in[col_p]) [* dinv_i]
// one kernel per sweep, the row's split taken from b_diag.  LANES = 1: one lane per row walks its part in stored order, a
// running subtraction.  LANES = 2, 4, 8: a group of lanes strides the part, the partial sums meet by shuffles and are
// subtracted from rhs_i once.  `in` and `out` are distinct buffers; in == NULL stands for an empty sum (z_0 = dinv .* y).
// hpcla_ilu_apply_f64 reads r in the lower sweeps only and writes out in the upper ones only, so its out may be its r.
#include "common.h"
#include "scan.h"

namespace hpcla {

constexpr int ILU_THREADS = 256;
constexpr unsigned long long ILU_NO_DIAG = 1, ILU_BAD_DIAG = 2, ILU_BAD_PIVOT = 3;

// owned entries of row i
template <typename I>
struct IluCountLoad {
    const I *a_rowptr, *a_colval;
    int base;
    int64_t n_own;
    __device__ int64_t operator()(int64_t i) const
    {
        const int64_t e0 = (int64_t)a_rowptr[i] - base, e1 = (int64_t)a_rowptr[i + 1] - base;
        int64_t m = 0;
        for (int64_t e = e0; e < e1; ++e) m += ((int64_t)a_colval[e] - base < n_own) ? 1 : 0;
        return m;
    }
};

struct IluCountEmit {
    int64_t nrows;
    int32_t *b_rowptr;
    int64_t *info;
    __device__ void operator()(int64_t i, int64_t before, int64_t m) const
    {
        b_rowptr[i] = (int32_t)before;
        if (i == nrows - 1) {
            b_rowptr[nrows] = (int32_t)(before + m);
            info[0] = before + m;
        }
    }
};

// One lane per row.  An owned entry's place in its row is the number of owned entries of the row with a smaller column (an
// earlier position breaks a tie): quadratic in the row's length, no scratch, any order of A's columns.
template <typename I>
__global__ __launch_bounds__(ILU_THREADS) void ilu_fill_kernel(const I *__restrict__ a_rowptr, const I *__restrict__ a_colval,
                                                               const double *__restrict__ a_nzval, int64_t nrows, int64_t n_own,
                                                               int base, const int32_t *__restrict__ b_rowptr,
                                                               int32_t *__restrict__ b_cols, int32_t *__restrict__ b_rows,
                                                               int32_t *__restrict__ b_diag, int64_t *__restrict__ b_map,
                                                               int64_t *__restrict__ info)
{
    const int64_t i = (int64_t)blockIdx.x * ILU_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int64_t e0 = (int64_t)a_rowptr[i] - base, e1 = (int64_t)a_rowptr[i + 1] - base;
    const int32_t out0 = b_rowptr[i];
    int32_t dp = -1;
    double dval = 1.0;
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t c = (int64_t)a_colval[e] - base;
        if (c >= n_own) continue;
        int32_t rank = 0;
        for (int64_t e2 = e0; e2 < e1; ++e2) {
            const int64_t c2 = (int64_t)a_colval[e2] - base;
            rank += (c2 < c || (c2 == c && e2 < e)) ? 1 : 0;    // a ghost is never below an owned column
        }
        const int32_t pos = out0 + rank;
        b_cols[pos] = (int32_t)c;
        b_rows[pos] = (int32_t)i;
        b_map[pos] = e;
        if (c == i) {
            dp = pos;
            dval = a_nzval[e];
        }
    }
    b_diag[i] = dp;
    unsigned long long *err = reinterpret_cast<unsigned long long *>(info + 1);
    if (dp < 0)
        atomicMin(err, ((unsigned long long)i << 2) | ILU_NO_DIAG);
    else if (dval == 0.0 || dval != dval)
        atomicMin(err, ((unsigned long long)i << 2) | ILU_BAD_DIAG);
}

static __global__ __launch_bounds__(ILU_THREADS) void ilu_gather_kernel(const double *__restrict__ a_nzval,
                                                                        const int64_t *__restrict__ b_map, int64_t nnz,
                                                                        double *__restrict__ a_vals)
{
    const int64_t p = (int64_t)blockIdx.x * ILU_THREADS + threadIdx.x;
    if (p < nnz) a_vals[p] = a_nzval[b_map[p]];
}

static __global__ __launch_bounds__(ILU_THREADS) void ilu_init_kernel(const int32_t *__restrict__ b_cols,
                                                                      const int32_t *__restrict__ b_rows,
                                                                      const int32_t *__restrict__ b_diag,
                                                                      const double *__restrict__ a_vals, int64_t nnz,
                                                                      double *__restrict__ f)
{
    const int64_t p = (int64_t)blockIdx.x * ILU_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const int32_t i = b_rows[p], j = b_cols[p];
    const double a = a_vals[p];
    if (i > j) {
        const int32_t dj = b_diag[j];
        f[p] = a / (dj >= 0 ? a_vals[dj] : __builtin_nan(""));
    } else {
        f[p] = a;
    }
}

// One lane per stored entry; the lanes of a wave take consecutive entries, which mostly share a row.
static __global__ __launch_bounds__(ILU_THREADS) void ilu_sweep_kernel(
    const int32_t *__restrict__ b_rowptr, const int32_t *__restrict__ b_cols, const int32_t *__restrict__ b_rows,
    const int32_t *__restrict__ b_diag, const int32_t *__restrict__ c_ptr, const int32_t *__restrict__ c_pos,
    const double *__restrict__ a_vals, const double *__restrict__ f_old, double *__restrict__ f_new, int64_t nnz)
{
    const int64_t p = (int64_t)blockIdx.x * ILU_THREADS + threadIdx.x;
    if (p >= nnz) return;
    const int32_t i = b_rows[p], j = b_cols[p];
    const int32_t m = i < j ? i : j;
    double s = a_vals[p];
    int32_t rp = b_rowptr[i], cq = c_ptr[j];
    const int32_t re = b_rowptr[i + 1], ce = c_ptr[j + 1];
    while (rp < re && cq < ce) {
        const int32_t q = c_pos[cq];
        const int32_t kr = b_cols[rp], kc = b_rows[q];
        if (kr >= m || kc >= m) break;
        if (kr == kc) {
            s = s - f_old[rp] * f_old[q];                       // l_ik * u_kj
            ++rp;
            ++cq;
        } else if (kr < kc) {
            ++rp;
        } else {
            ++cq;
        }
    }
    if (i > j) {
        const int32_t dj = b_diag[j];
        f_new[p] = s / (dj >= 0 ? f_old[dj] : __builtin_nan(""));
    } else {
        f_new[p] = s;
    }
}

static __global__ __launch_bounds__(ILU_THREADS) void ilu_pivots_kernel(const int32_t *__restrict__ b_diag,
                                                                        const double *__restrict__ f, int64_t nrows,
                                                                        double *__restrict__ dinv, int64_t *__restrict__ info)
{
    const int64_t i = (int64_t)blockIdx.x * ILU_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int32_t dp = b_diag[i];
    const double u = dp >= 0 ? f[dp] : __builtin_nan("");
    dinv[i] = 1.0 / u;
    if (dp >= 0 && (u == 0.0 || u != u || u - u != 0.0))        // zero, NaN, infinite
        atomicMin(reinterpret_cast<unsigned long long *>(info + 1), ((unsigned long long)i << 2) | ILU_BAD_PIVOT);
}

template <int LANES>
__global__ __launch_bounds__(ILU_THREADS) void ilu_trisweep_kernel(const int32_t *__restrict__ b_rowptr,
                                                                   const int32_t *__restrict__ b_cols,
                                                                   const int32_t *__restrict__ b_diag,
                                                                   const double *__restrict__ f, const double *__restrict__ rhs,
                                                                   const double *__restrict__ in, const double *__restrict__ dinv,
                                                                   double *__restrict__ out, int64_t nrows, int upper)
{
    const int64_t t = (int64_t)blockIdx.x * ILU_THREADS + threadIdx.x;
    const int64_t i = t / LANES;
    const int sub = (int)(t % LANES);
    const bool live = i < nrows;
    int32_t lo = 0, hi = 0;
    if (live && in) {
        const int32_t dp = b_diag[i];
        lo = upper ? dp + 1 : b_rowptr[i];
        hi = upper ? b_rowptr[i + 1] : dp;
    }
    double acc;
    if (LANES == 1) {
        acc = live ? rhs[i] : 0.0;
        for (int32_t p = lo; p < hi; ++p) acc = acc - f[p] * in[b_cols[p]];
    } else {
        double part = 0.0;
        for (int32_t p = lo + sub; p < hi; p += LANES) part = part + f[p] * in[b_cols[p]];
#pragma unroll
        for (int off = LANES / 2; off >= 1; off >>= 1) part = part + __shfl_xor(part, off, LANES);
        acc = (live ? rhs[i] : 0.0) - part;
    }
    if (live && sub == 0) out[i] = dinv ? acc * dinv[i] : acc;
}

template <typename I>
static int ilu_count_impl(const I *a_rowptr, const I *a_colval, int64_t nrows, int64_t n_own, int index_base, int32_t *b_rowptr,
                          int64_t *info, void *work, void *stream)
{
    if (nrows < 0 || n_own != nrows) return set_error(HPCLA_ERR_INVALID, "ilu_count: needs n_own == nrows >= 0");
    if (nrows >= 0x7fffffffLL) return set_error(HPCLA_ERR_UNSUPPORTED, "ilu_count: needs nrows < 2^31 - 1");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "ilu_count: index_base must be 0 or 1");
    if (!b_rowptr || !info || !work) return set_error(HPCLA_ERR_INVALID, "ilu_count: null rowptr / info / work");
    if (nrows > 0 && (!a_rowptr || !a_colval)) return set_error(HPCLA_ERR_INVALID, "ilu_count: null CSR array");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(info, 0, sizeof(int64_t), s));
    HPCLA_CHECK_HIP(hipMemsetAsync(info + 1, 0xff, sizeof(int64_t), s));
    if (nrows == 0) {
        HPCLA_CHECK_HIP(hipMemsetAsync(b_rowptr, 0, sizeof(int32_t), s));
        return HPCLA_OK;
    }
    int64_t *sums = reinterpret_cast<int64_t *>(work);
    return exclusive_scan(IluCountLoad<I>{a_rowptr, a_colval, index_base, n_own}, nrows, IluCountEmit{nrows, b_rowptr, info},
                          sums + 1, sums, s);
}

template <typename I>
static int ilu_fill_impl(const I *a_rowptr, const I *a_colval, const double *a_nzval, int64_t nrows, int64_t n_own,
                         int index_base, const int32_t *b_rowptr, int32_t *b_cols, int32_t *b_rows, int32_t *b_diag,
                         int64_t *b_map, int64_t *info, void *stream)
{
    if (nrows < 0 || n_own != nrows) return set_error(HPCLA_ERR_INVALID, "ilu_fill: needs n_own == nrows >= 0");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "ilu_fill: index_base must be 0 or 1");
    if (!info) return set_error(HPCLA_ERR_INVALID, "ilu_fill: null info");
    if (nrows == 0) return HPCLA_OK;
    if (!a_rowptr || !a_colval || !a_nzval || !b_rowptr || !b_cols || !b_rows || !b_diag || !b_map)
        return set_error(HPCLA_ERR_INVALID, "ilu_fill: null array");
    const int64_t nb = (nrows + ILU_THREADS - 1) / ILU_THREADS;
    HPCLA_CHECK_GRID(nb, "ilu_fill");
    ilu_fill_kernel<I><<<(uint32_t)nb, ILU_THREADS, 0, as_stream(stream)>>>(a_rowptr, a_colval, a_nzval, nrows, n_own, index_base,
                                                                           b_rowptr, b_cols, b_rows, b_diag, b_map, info);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

static int ilu_trisweep_launch(const int32_t *b_rowptr, const int32_t *b_cols, const int32_t *b_diag, const double *f,
                               const double *rhs, const double *in, const double *dinv, double *out, int64_t nrows, int upper,
                               int lanes, hipStream_t s)
{
    const int64_t nb = (nrows * lanes + ILU_THREADS - 1) / ILU_THREADS;
    HPCLA_CHECK_GRID(nb, "ilu_trisweep");
#define HPCLA_ILU_TRISWEEP(L) \
    ilu_trisweep_kernel<L><<<(uint32_t)nb, ILU_THREADS, 0, s>>>(b_rowptr, b_cols, b_diag, f, rhs, in, dinv, out, nrows, upper)
    switch (lanes) {
    case 1: HPCLA_ILU_TRISWEEP(1); break;
    case 2: HPCLA_ILU_TRISWEEP(2); break;
    case 4: HPCLA_ILU_TRISWEEP(4); break;
    default: HPCLA_ILU_TRISWEEP(8); break;
    }
#undef HPCLA_ILU_TRISWEEP
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

static bool ilu_lanes_ok(int lanes) { return lanes == 1 || lanes == 2 || lanes == 4 || lanes == 8; }

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_ilu_work_bytes(int64_t nrows)
{
    if (nrows < 0) return -1;
    return (int64_t)sizeof(int64_t) * (1 + scan_blocks(nrows > 0 ? nrows : 1));
}

HPCLA_API int hpcla_ilu_count_f64_i32(const int32_t *a_rowptr, const int32_t *a_colval_split, int64_t nrows, int64_t n_own,
                                      int index_base, int32_t *b_rowptr_dev, int64_t *info_dev, void *work, void *stream)
{
    return ilu_count_impl<int32_t>(a_rowptr, a_colval_split, nrows, n_own, index_base, b_rowptr_dev, info_dev, work, stream);
}

HPCLA_API int hpcla_ilu_count_f64_i64(const int64_t *a_rowptr, const int64_t *a_colval_split, int64_t nrows, int64_t n_own,
                                      int index_base, int32_t *b_rowptr_dev, int64_t *info_dev, void *work, void *stream)
{
    return ilu_count_impl<int64_t>(a_rowptr, a_colval_split, nrows, n_own, index_base, b_rowptr_dev, info_dev, work, stream);
}

HPCLA_API int hpcla_ilu_fill_f64_i32(const int32_t *a_rowptr, const int32_t *a_colval_split, const double *a_nzval, int64_t nrows,
                                     int64_t n_own, int index_base, const int32_t *b_rowptr_dev, int32_t *b_cols_dev,
                                     int32_t *b_rows_dev, int32_t *b_diag_dev, int64_t *b_map_dev, int64_t *info_dev,
                                     void *stream)
{
    return ilu_fill_impl<int32_t>(a_rowptr, a_colval_split, a_nzval, nrows, n_own, index_base, b_rowptr_dev, b_cols_dev,
                                  b_rows_dev, b_diag_dev, b_map_dev, info_dev, stream);
}

HPCLA_API int hpcla_ilu_fill_f64_i64(const int64_t *a_rowptr, const int64_t *a_colval_split, const double *a_nzval, int64_t nrows,
                                     int64_t n_own, int index_base, const int32_t *b_rowptr_dev, int32_t *b_cols_dev,
                                     int32_t *b_rows_dev, int32_t *b_diag_dev, int64_t *b_map_dev, int64_t *info_dev,
                                     void *stream)
{
    return ilu_fill_impl<int64_t>(a_rowptr, a_colval_split, a_nzval, nrows, n_own, index_base, b_rowptr_dev, b_cols_dev,
                                  b_rows_dev, b_diag_dev, b_map_dev, info_dev, stream);
}

HPCLA_API int hpcla_ilu_gather_f64(const double *a_nzval, const int64_t *b_map_dev, int64_t nnz, double *a_vals_dev, void *stream)
{
    if (nnz < 0) return set_error(HPCLA_ERR_INVALID, "ilu_gather: negative size");
    if (nnz == 0) return HPCLA_OK;
    if (!a_nzval || !b_map_dev || !a_vals_dev) return set_error(HPCLA_ERR_INVALID, "ilu_gather: null array");
    const int64_t nb = (nnz + ILU_THREADS - 1) / ILU_THREADS;
    HPCLA_CHECK_GRID(nb, "ilu_gather");
    ilu_gather_kernel<<<(uint32_t)nb, ILU_THREADS, 0, as_stream(stream)>>>(a_nzval, b_map_dev, nnz, a_vals_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_ilu_init_f64(const int32_t *b_cols_dev, const int32_t *b_rows_dev, const int32_t *b_diag_dev,
                                 const double *a_vals_dev, int64_t nnz, double *f_dev, void *stream)
{
    if (nnz < 0 || nnz > 0x7fffffffLL) return set_error(HPCLA_ERR_INVALID, "ilu_init: needs 0 <= nnz < 2^31");
    if (nnz == 0) return HPCLA_OK;
    if (!b_cols_dev || !b_rows_dev || !b_diag_dev || !a_vals_dev || !f_dev) return set_error(HPCLA_ERR_INVALID, "ilu_init: null array");
    const int64_t nb = (nnz + ILU_THREADS - 1) / ILU_THREADS;
    ilu_init_kernel<<<(uint32_t)nb, ILU_THREADS, 0, as_stream(stream)>>>(b_cols_dev, b_rows_dev, b_diag_dev, a_vals_dev, nnz, f_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_ilu_sweep_f64(const int32_t *b_rowptr_dev, const int32_t *b_cols_dev, const int32_t *b_rows_dev,
                                  const int32_t *b_diag_dev, const int32_t *c_ptr_dev, const int32_t *c_pos_dev,
                                  const double *a_vals_dev, const double *f_old_dev, double *f_new_dev, int64_t nnz, void *stream)
{
    if (nnz < 0 || nnz > 0x7fffffffLL) return set_error(HPCLA_ERR_INVALID, "ilu_sweep: needs 0 <= nnz < 2^31");
    if (nnz == 0) return HPCLA_OK;
    if (!b_rowptr_dev || !b_cols_dev || !b_rows_dev || !b_diag_dev || !c_ptr_dev || !c_pos_dev || !a_vals_dev || !f_old_dev ||
        !f_new_dev)
        return set_error(HPCLA_ERR_INVALID, "ilu_sweep: null array");
    if (f_old_dev == f_new_dev) return set_error(HPCLA_ERR_INVALID, "ilu_sweep: the old and the new values must be two buffers");
    const int64_t nb = (nnz + ILU_THREADS - 1) / ILU_THREADS;
    ilu_sweep_kernel<<<(uint32_t)nb, ILU_THREADS, 0, as_stream(stream)>>>(b_rowptr_dev, b_cols_dev, b_rows_dev, b_diag_dev,
                                                                         c_ptr_dev, c_pos_dev, a_vals_dev, f_old_dev, f_new_dev,
                                                                         nnz);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_ilu_pivots_f64(const int32_t *b_diag_dev, const double *f_dev, int64_t nrows, double *dinv_dev,
                                   int64_t *info_dev, void *stream)
{
    if (nrows < 0) return set_error(HPCLA_ERR_INVALID, "ilu_pivots: negative size");
    if (!info_dev) return set_error(HPCLA_ERR_INVALID, "ilu_pivots: null info");
    if (nrows == 0) return HPCLA_OK;
    if (!b_diag_dev || !f_dev || !dinv_dev) return set_error(HPCLA_ERR_INVALID, "ilu_pivots: null array");
    const int64_t nb = (nrows + ILU_THREADS - 1) / ILU_THREADS;
    HPCLA_CHECK_GRID(nb, "ilu_pivots");
    ilu_pivots_kernel<<<(uint32_t)nb, ILU_THREADS, 0, as_stream(stream)>>>(b_diag_dev, f_dev, nrows, dinv_dev, info_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_ilu_trisweep_f64(const int32_t *b_rowptr_dev, const int32_t *b_cols_dev, const int32_t *b_diag_dev,
                                     const double *f_dev, const double *rhs, const double *in, const double *dinv_dev,
                                     double *out, int64_t nrows, int upper, int lanes, void *stream)
{
    if (nrows < 0) return set_error(HPCLA_ERR_INVALID, "ilu_trisweep: negative size");
    if (!ilu_lanes_ok(lanes)) return set_error(HPCLA_ERR_INVALID, "ilu_trisweep: lanes must be 1, 2, 4 or 8");
    if (nrows == 0) return HPCLA_OK;
    if (!b_rowptr_dev || !b_cols_dev || !b_diag_dev || !f_dev || !rhs || !out)
        return set_error(HPCLA_ERR_INVALID, "ilu_trisweep: null array");
    if (in == out) return set_error(HPCLA_ERR_INVALID, "ilu_trisweep: in and out must be two buffers");
    return ilu_trisweep_launch(b_rowptr_dev, b_cols_dev, b_diag_dev, f_dev, rhs, in, dinv_dev, out, nrows, upper ? 1 : 0, lanes,
                               as_stream(stream));
}

HPCLA_API int hpcla_ilu_apply_f64(const int32_t *b_rowptr_dev, const int32_t *b_cols_dev, const int32_t *b_diag_dev,
                                  const double *f_dev, const double *dinv_dev, const double *r, double *t0, double *t1, double *out,
                                  int64_t nrows, int solve_sweeps, int lanes, void *stream)
{
    if (nrows < 0) return set_error(HPCLA_ERR_INVALID, "ilu_apply: negative size");
    if (solve_sweeps < 1 || solve_sweeps > 16) return set_error(HPCLA_ERR_INVALID, "ilu_apply: solve_sweeps must be in 1..16");
    if (!ilu_lanes_ok(lanes)) return set_error(HPCLA_ERR_INVALID, "ilu_apply: lanes must be 1, 2, 4 or 8");
    if (nrows == 0) return HPCLA_OK;
    if (!b_rowptr_dev || !b_cols_dev || !b_diag_dev || !f_dev || !dinv_dev || !r || !t0 || !t1 || !out)
        return set_error(HPCLA_ERR_INVALID, "ilu_apply: null array");
    if (t0 == t1 || t0 == out || t1 == out || r == t0 || r == t1)
        return set_error(HPCLA_ERR_INVALID, "ilu_apply: t0 and t1 must be distinct from each other, from r and from out");
    hipStream_t s = as_stream(stream);
    double *t[2] = {t0, t1};
    // y_0 = r, y_{m+1} = r - L y_m: the sweeps land in t0, t1, t0, ...
    const double *in = r;
    for (int m = 0; m < solve_sweeps; ++m) {
        double *o = t[m & 1];
        if (int rc = ilu_trisweep_launch(b_rowptr_dev, b_cols_dev, b_diag_dev, f_dev, r, in, nullptr, o, nrows, 0, lanes, s)) return rc;
        in = o;
    }
    const double *y = in;
    double *spare = t[solve_sweeps & 1];                        // the one of t0, t1 that does not hold y
    // z_0 = dinv .* y, z_{m+1} = dinv .* (y - U z_m): solve_sweeps + 1 launches that alternate and end in out
    in = nullptr;
    for (int m = 0; m <= solve_sweeps; ++m) {
        double *o = ((solve_sweeps - m) & 1) ? spare : out;
        if (int rc = ilu_trisweep_launch(b_rowptr_dev, b_cols_dev, b_diag_dev, f_dev, y, in, dinv_dev, o, nrows, 1, lanes, s)) return rc;
        in = o;
    }
    return HPCLA_OK;
}
