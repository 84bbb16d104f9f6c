// spmm_t.hip -- transposed SpMM, W = A^T X, for the dense-times-sparse products transpose(X) * A and X * A (gfx950).
//
// Reference: `transpose(X) * A` and `X * A` with A sparse (src/sparse.jl:3617-3690) loop over the n columns of A: for each
// column one sparse column extraction across ranks, one dense mat-vec with its own all-reduce and one copy to the host.
// Here the product is one pass over this rank's rows of A and X:
//
//   * STRUCTURE (once per sparse structure, memoised by the callers under the structural hash): a local CSC of this rank's
//     rows over the split column space (own columns first, then the ghost segments, as the SpMV plan numbers them) --
//     colptr_t, rowidx_t (local row, ascending in each column) and perm (CSC position -> CSR position).  Built on the device
//     by a stable radix sort of the CSR positions keyed by column (rocPRIM, header-only: a sequence of counting sorts), so
//     equal columns keep their stored order.  (A one-pass counting sort needs each entry's rank among the earlier entries
//     of its column; with atomics that rank depends on timing, and the stable form is exactly a radix sort's passes.)  No
//     copy of the values: `2 * A` shares A's structure and has new nzval, and the
//     product gathers nzval through perm on every call.
//   * PRODUCT: W[c, :] = sum over e in [colptr_t[c], colptr_t[c+1]) of nzval[perm[e]] * X[rowidx_t[e], :], one running sum
//     per (column, X column) that starts at 0.0 and adds the products in ascending row order with separate multiply and
//     add (-ffp-contract=off): the bits of the SpMM over the materialised A^T (spmm.hip), the order of the reference's
//     stored-order row sums.  No atomics.  X is read as rows (one 128-byte line per entry at m = 16); W is written row- or
//     column-major.
//   * REVERSE HALO (N > 1): the ghost rows of W are partial sums of other ranks' columns; they travel back to their owners
//     through hpcla_exchange_ranges_f64 and hpcla_spmm_t_accumulate_f64 adds them to the owner's rows in a fixed order.
//
// Mapping of the product: LPC lanes per compressed column, two X columns per lane (a 16-byte load when the rows allow it),
// 256 / LPC columns per workgroup; the workgroup's CSC range (entries of consecutive columns are consecutive) is staged
// through LDS as (X row offset, value) records, as the SpMM stages its CSR range.  A column-major W leaves through LDS as
// runs along the column index.
#include <limits>
#include <type_traits>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"

namespace hpcla {

namespace {

constexpr int TPB_T = 256;
constexpr int CHUNK_T = 1024;               // records staged per pass: 16 KiB of LDS (+ 4 KiB for the W tile): 8 workgroups per CU

typedef double vdouble2 __attribute__((ext_vector_type(2)));

inline int64_t align_up(int64_t b) { return (b + 255) & ~(int64_t)255; }

// ---- structure -------------------------------------------------------------------------------------------------------------
template <typename I>
__global__ __launch_bounds__(256) void iota_kernel(I *__restrict__ out, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (I)i;
}

// colptr[c] = first sorted position whose key is >= c, for c in [0, ncols]: one binary search per column, so a rank with
// few stored entries and many columns fills its colptr in parallel like any other
template <typename U, typename I>
__global__ __launch_bounds__(256) void colptr_kernel(const U *__restrict__ keys, int64_t nnz, int64_t ncols, I *__restrict__ colptr)
{
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= ncols; c += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = nnz;                      // keys[0 .. lo) < c <= keys[hi .. nnz)
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)keys[mid] < c) lo = mid + 1;
            else hi = mid;
        }
        colptr[c] = (I)lo;
    }
}

// rowidx[e] = the local row of CSR position perm[e] (the last row whose rowptr entry is <= it)
template <typename I>
__global__ __launch_bounds__(256) void rowidx_kernel(const I *__restrict__ rowptr, int64_t nrows, const I *__restrict__ perm,
                                                     I *__restrict__ rowidx, int64_t nnz)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = (int64_t)perm[e];
        int64_t lo = 0, hi = nrows;                    // rowptr[lo] <= p < rowptr[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)rowptr[mid] <= p) lo = mid;
            else hi = mid;
        }
        rowidx[e] = (I)lo;
    }
}

inline uint32_t grid_of(int64_t n)
{
    const int64_t b = (n + 255) / 256;
    return (uint32_t)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

inline int key_bits(int64_t ncols)
{
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) < ncols) ++b;
    return b;
}

template <typename I>
int64_t struct_work_bytes(int64_t nnz, int64_t ncols)
{
    typedef typename std::make_unsigned<I>::type U;
    size_t tmp = 0;
    if (nnz > 0 && rocprim::radix_sort_pairs((void *)nullptr, tmp, (const U *)nullptr, (U *)nullptr, (const I *)nullptr,
                                             (I *)nullptr, (size_t)nnz, 0, key_bits(ncols)) != hipSuccess)
        return -1;
    return 2 * align_up(nnz * (int64_t)sizeof(I)) + align_up((int64_t)tmp) + 256;
}

template <typename I>
int struct_impl(const I *rowptr, const I *colval, int64_t nrows, int64_t nnz, int64_t ncols, I *colptr_t, I *rowidx_t, I *perm,
                void *work, int64_t work_bytes, void *stream, const char *who)
{
    typedef typename std::make_unsigned<I>::type U;
    if (nrows < 0 || nnz < 0 || ncols < 0) return set_error(HPCLA_ERR_INVALID, "%s: negative size", who);
    if (!colptr_t) return set_error(HPCLA_ERR_INVALID, "%s: null colptr_t", who);
    if (nnz > 0 && (!rowptr || !colval || !rowidx_t || !perm || !work))
        return set_error(HPCLA_ERR_INVALID, "%s: null array with nnz > 0", who);
    if ((int64_t)std::numeric_limits<I>::max() < (nnz > ncols ? nnz : ncols))
        return set_error(HPCLA_ERR_UNSUPPORTED, "%s: sizes do not fit the index type", who);
    hipStream_t s = as_stream(stream);
    if (nnz == 0) {
        colptr_kernel<U, I><<<grid_of(ncols + 1), 256, 0, s>>>(nullptr, 0, ncols, colptr_t);
        HPCLA_CHECK_LAUNCH();
        return HPCLA_OK;
    }
    const int64_t need = struct_work_bytes<I>(nnz, ncols);
    if (need < 0) return set_error(HPCLA_ERR_HIP, "%s: sort workspace query failed", who);
    if (work_bytes < need) return set_error(HPCLA_ERR_INVALID, "%s: work buffer too small (%lld < %lld bytes)", who,
                                            (long long)work_bytes, (long long)need);
    char *base = reinterpret_cast<char *>(((uintptr_t)work + 255) & ~(uintptr_t)255);
    I *pos_in = reinterpret_cast<I *>(base);
    U *keys_out = reinterpret_cast<U *>(base + align_up(nnz * (int64_t)sizeof(I)));
    void *tmp = base + 2 * align_up(nnz * (int64_t)sizeof(I));
    size_t tmp_bytes = (size_t)(need - 256 - 2 * align_up(nnz * (int64_t)sizeof(I)));
    iota_kernel<I><<<grid_of(nnz), 256, 0, s>>>(pos_in, nnz);
    HPCLA_CHECK_LAUNCH();
    // stable: positions with equal columns stay ascending, i.e. in ascending row and stored order
    HPCLA_CHECK_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, reinterpret_cast<const U *>(colval), keys_out, pos_in, perm,
                                              (size_t)nnz, 0, key_bits(ncols), s));
    colptr_kernel<U, I><<<grid_of(ncols + 1), 256, 0, s>>>(keys_out, nnz, ncols, colptr_t);
    HPCLA_CHECK_LAUNCH();
    rowidx_kernel<I><<<grid_of(nnz), 256, 0, s>>>(rowptr, nrows, perm, rowidx_t, nnz);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// ---- product ---------------------------------------------------------------------------------------------------------------
// VEC: X rows are 16-byte aligned with unit column stride and m is even (a lane's two columns are one vdouble2).
// WCOL: W has unit row stride (column-major): the tile leaves through LDS as runs along the column index.
template <typename I, int LPC, bool VEC, bool WCOL>
__global__ __launch_bounds__(TPB_T) void spmm_t_kernel(const I *__restrict__ colptr, const I *__restrict__ rowidx,
                                                       const I *__restrict__ perm, const double *__restrict__ nzval, int64_t ncols,
                                                       const double *__restrict__ X, int64_t x_rs, int64_t x_cs, int64_t m,
                                                       double *__restrict__ W, int64_t w_rs, int64_t w_cs)
{
    constexpr int CPB = TPB_T / LPC, KTILE = 2 * LPC;
    __shared__ int64_t s_off[CHUNK_T];
    __shared__ double s_val[CHUNK_T];
    __shared__ double s_out[WCOL ? KTILE * CPB : 1];
    const int tid = threadIdx.x, g = tid / LPC, l = tid % LPC;
    const int64_t c0 = (int64_t)blockIdx.x * CPB;
    const int nc = (int)((ncols - c0) < CPB ? (ncols - c0) : CPB);
    const int64_t p0 = (int64_t)colptr[c0];
    const int64_t total = (int64_t)colptr[c0 + nc] - p0;
    int64_t lo = 0, hi = 0;                              // this lane-group's column, relative to p0
    if (g < nc) {
        lo = (int64_t)colptr[c0 + g] - p0;
        hi = (int64_t)colptr[c0 + g + 1] - p0;
    }
    const bool single = total <= CHUNK_T;
    if (single) {
        for (int i = tid; i < (int)total; i += TPB_T) {
            s_off[i] = (int64_t)rowidx[p0 + i] * x_rs;
            s_val[i] = nzval[(int64_t)perm[p0 + i]];
        }
        __syncthreads();
    }
    for (int64_t kt = 0; kt < m; kt += KTILE) {
        const int64_t c = kt + 2 * l;
        const bool two = c + 1 < m;
        double a0 = 0.0, a1 = 0.0;
        for (int64_t ch = 0; ch < total; ch += CHUNK_T) {
            const int n = (int)((total - ch) < CHUNK_T ? (total - ch) : CHUNK_T);
            if (!single) {
                __syncthreads();                         // the previous pass is done with LDS
                for (int i = tid; i < n; i += TPB_T) {
                    s_off[i] = (int64_t)rowidx[p0 + ch + i] * x_rs;
                    s_val[i] = nzval[(int64_t)perm[p0 + ch + i]];
                }
                __syncthreads();
            }
            const int64_t b = lo > ch ? lo : ch, e = hi < ch + n ? hi : ch + n;
            if (c < m) {
                const double *xc = X + c * x_cs;
                for (int64_t i = b - ch; i < e - ch; ++i) {
                    const double v = s_val[i];
                    if (VEC) {
                        const vdouble2 x = *reinterpret_cast<const vdouble2 *>(xc + s_off[i]);
                        a0 = a0 + v * x.x;
                        a1 = a1 + v * x.y;
                    } else {
                        a0 = a0 + v * xc[s_off[i]];
                        if (two) a1 = a1 + v * xc[s_off[i] + x_cs];
                    }
                }
            }
        }
        if (!WCOL) {
            if (g < nc && c < m) {
                double *w = W + (c0 + g) * w_rs + c * w_cs;
                w[0] = a0;
                if (two) w[w_cs] = a1;
            }
        } else {
            s_out[(2 * l) * CPB + g] = a0;
            s_out[(2 * l + 1) * CPB + g] = a1;
            __syncthreads();
            for (int i = tid; i < KTILE * CPB; i += TPB_T) {
                const int j = i / CPB, cc = i - j * CPB;
                if (cc < nc && kt + j < m) W[(c0 + cc) + (kt + j) * w_cs] = s_out[i];
            }
            __syncthreads();                             // the tile is read before the next one is parked
        }
    }
}

template <typename I>
int spmm_t_impl(const I *colptr, const I *rowidx, const I *perm, const double *nzval, int64_t ncols, const double *X, int64_t ldx,
                int x_layout, int64_t m, double *W, int64_t ldw, int w_layout, void *stream, const char *who)
{
    if (ncols < 0 || m < 0) return set_error(HPCLA_ERR_INVALID, "%s: negative size", who);
    if ((x_layout != HPCLA_LAYOUT_ROW && x_layout != HPCLA_LAYOUT_COL) || (w_layout != HPCLA_LAYOUT_ROW && w_layout != HPCLA_LAYOUT_COL))
        return set_error(HPCLA_ERR_INVALID, "%s: layout must be HPCLA_LAYOUT_ROW or HPCLA_LAYOUT_COL", who);
    if (ncols == 0 || m == 0) return HPCLA_OK;
    if (!colptr || !W) return set_error(HPCLA_ERR_INVALID, "%s: null colptr / W", who);
    if (w_layout == HPCLA_LAYOUT_ROW ? ldw < m : ldw < ncols) return set_error(HPCLA_ERR_INVALID, "%s: ldw too small", who);
    if (x_layout == HPCLA_LAYOUT_ROW && ldx < m) return set_error(HPCLA_ERR_INVALID, "%s: ldx too small", who);
    const int64_t x_rs = x_layout == HPCLA_LAYOUT_ROW ? ldx : 1, x_cs = x_layout == HPCLA_LAYOUT_ROW ? 1 : ldx;
    const int64_t w_rs = w_layout == HPCLA_LAYOUT_ROW ? ldw : 1, w_cs = w_layout == HPCLA_LAYOUT_ROW ? 1 : ldw;
    // (rowidx / perm / nzval / X are read only where colptr has entries: a rank without stored entries may pass NULL)
    const bool vec = x_cs == 1 && (x_rs & 1) == 0 && (m & 1) == 0 && ((uintptr_t)X & 15) == 0;
    const bool wcol = w_layout == HPCLA_LAYOUT_COL;
    const int lpc = m <= 2 ? 1 : m <= 4 ? 2 : m <= 8 ? 4 : m <= 16 ? 8 : m <= 32 ? 16 : 32;
    const int64_t nb = (ncols + (TPB_T / lpc) - 1) / (TPB_T / lpc);
    HPCLA_CHECK_GRID(nb, who);
    hipStream_t s = as_stream(stream);
#define HPCLA_SPMM_T(LPC)                                                                                                          \
    do {                                                                                                                          \
        if (vec && wcol) spmm_t_kernel<I, LPC, true, true><<<(uint32_t)nb, TPB_T, 0, s>>>(colptr, rowidx, perm, nzval, ncols, X, \
                                                                                          x_rs, x_cs, m, W, w_rs, w_cs);          \
        else if (vec) spmm_t_kernel<I, LPC, true, false><<<(uint32_t)nb, TPB_T, 0, s>>>(colptr, rowidx, perm, nzval, ncols, X,  \
                                                                                        x_rs, x_cs, m, W, w_rs, w_cs);            \
        else if (wcol) spmm_t_kernel<I, LPC, false, true><<<(uint32_t)nb, TPB_T, 0, s>>>(colptr, rowidx, perm, nzval, ncols, X, \
                                                                                          x_rs, x_cs, m, W, w_rs, w_cs);          \
        else spmm_t_kernel<I, LPC, false, false><<<(uint32_t)nb, TPB_T, 0, s>>>(colptr, rowidx, perm, nzval, ncols, X, x_rs,    \
                                                                                 x_cs, m, W, w_rs, w_cs);                         \
    } while (0)
    switch (lpc) {
    case 1: HPCLA_SPMM_T(1); break;
    case 2: HPCLA_SPMM_T(2); break;
    case 4: HPCLA_SPMM_T(4); break;
    case 8: HPCLA_SPMM_T(8); break;
    case 16: HPCLA_SPMM_T(16); break;
    default: HPCLA_SPMM_T(32); break;
    }
#undef HPCLA_SPMM_T
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// ---- reverse halo: V[rows[u], :] += R[pos[t], :] for t in [ptr[u], ptr[u+1]), in list order ------------------------------
__global__ __launch_bounds__(256) void accumulate_kernel(double *__restrict__ V, int64_t ldv, const double *__restrict__ R,
                                                         int64_t ldr, const int64_t *__restrict__ rows,
                                                         const int64_t *__restrict__ ptr, const int64_t *__restrict__ pos,
                                                         int64_t n_rows, int64_t m)
{
    const int64_t total = n_rows * m;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = i / m, j = i - u * m;
        double *v = V + rows[u] * ldv + j;
        double acc = *v;
        for (int64_t t = ptr[u]; t < ptr[u + 1]; ++t) acc = acc + R[pos[t] * ldr + j];
        *v = acc;
    }
}

}  // namespace

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_spmm_t_struct_work_bytes(int64_t nnz, int64_t ncols, int index_is_i64)
{
    if (nnz < 0 || ncols < 0) return -1;
    return index_is_i64 ? struct_work_bytes<int64_t>(nnz, ncols) : struct_work_bytes<int32_t>(nnz, ncols);
}

HPCLA_API int hpcla_spmm_t_struct_i32(const int32_t *rowptr, const int32_t *colval, int64_t nrows, int64_t nnz, int64_t ncols,
                                      int32_t *colptr_t, int32_t *rowidx_t, int32_t *perm, void *work, int64_t work_bytes,
                                      void *stream)
{
    return struct_impl<int32_t>(rowptr, colval, nrows, nnz, ncols, colptr_t, rowidx_t, perm, work, work_bytes, stream,
                                "hpcla_spmm_t_struct_i32");
}

HPCLA_API int hpcla_spmm_t_struct_i64(const int64_t *rowptr, const int64_t *colval, int64_t nrows, int64_t nnz, int64_t ncols,
                                      int64_t *colptr_t, int64_t *rowidx_t, int64_t *perm, void *work, int64_t work_bytes,
                                      void *stream)
{
    return struct_impl<int64_t>(rowptr, colval, nrows, nnz, ncols, colptr_t, rowidx_t, perm, work, work_bytes, stream,
                                "hpcla_spmm_t_struct_i64");
}

HPCLA_API int hpcla_spmm_t_f64_i32(const int32_t *colptr_t, const int32_t *rowidx_t, const int32_t *perm, const double *nzval,
                                   int64_t ncols, const double *X, int64_t ldx, int x_layout, int64_t m, double *W, int64_t ldw,
                                   int w_layout, void *stream)
{
    return spmm_t_impl<int32_t>(colptr_t, rowidx_t, perm, nzval, ncols, X, ldx, x_layout, m, W, ldw, w_layout, stream,
                                "hpcla_spmm_t_f64_i32");
}

HPCLA_API int hpcla_spmm_t_f64_i64(const int64_t *colptr_t, const int64_t *rowidx_t, const int64_t *perm, const double *nzval,
                                   int64_t ncols, const double *X, int64_t ldx, int x_layout, int64_t m, double *W, int64_t ldw,
                                   int w_layout, void *stream)
{
    return spmm_t_impl<int64_t>(colptr_t, rowidx_t, perm, nzval, ncols, X, ldx, x_layout, m, W, ldw, w_layout, stream,
                                "hpcla_spmm_t_f64_i64");
}

HPCLA_API int hpcla_spmm_t_accumulate_f64(double *V, int64_t ldv, const double *R, int64_t ldr, const int64_t *rows,
                                          const int64_t *ptr, const int64_t *pos, int64_t n_rows, int64_t m, void *stream)
{
    if (n_rows < 0 || m < 0) return set_error(HPCLA_ERR_INVALID, "hpcla_spmm_t_accumulate_f64: negative size");
    if (n_rows == 0 || m == 0) return HPCLA_OK;
    if (!V || !R || !rows || !ptr || !pos) return set_error(HPCLA_ERR_INVALID, "hpcla_spmm_t_accumulate_f64: null pointer");
    if (ldv < m || ldr < m) return set_error(HPCLA_ERR_INVALID, "hpcla_spmm_t_accumulate_f64: leading dimension < m");
    accumulate_kernel<<<grid_of(n_rows * m), 256, 0, as_stream(stream)>>>(V, ldv, R, ldr, rows, ptr, pos, n_rows, m);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}
