// submatrix.hip -- range indexing of a sparse matrix on the device: A[r0:r1, c0:c1] and A[:, k].
//
// Reference (host, entry by entry): Base.getindex(A::HPCSparseMatrix, ::UnitRange, ::UnitRange) walks `_get_csc(A)`,
// pushes the kept entries into growing lists, sorts every row and searches every entry in the list of kept columns
// (src/indexing.jl:691-840); Base.getindex(A, :, k) scans every row for one column (src/indexing.jl:872-914).  On a device
// backend both are scalar indexing of device arrays, or a round trip of the whole matrix through the host.
//
// Here the operation is what it is underneath: a copy.  It relies on two invariants of the struct.  `col_indices` is sorted,
// so the global column window [c0, c1) is ONE contiguous window [j0, j1) of compressed local columns (the caller finds it
// with two binary searches on the host).  Columns ascend within a row (src/sparse.jl:288-295), so the
// kept entries of a row are ONE contiguous run of its stored entries: a start and a count describe it, nothing is sorted,
// and stored order is kept.  Values are moved, never computed with: the kernels are templated on the element SIZE (4 or 8
// bytes) and copy integers, so -0.0, NaN payloads, Inf, denormals and explicit zeros keep every bit.
//
// Passes (all on the caller's stream):
//   locate  one lane per selected row, two lower-bound searches in the row: source start and count of its run.  Each lane
//           touches O(log len) scattered words -- uncoalesced by nature (cdna_hip_programming.md, Guideline 2 and Appendix B
//           "Scatter / gather"), but it moves 16 bytes per ROW; the pass that moves bytes per ENTRY is the fill, and that is
//           the one that must be coalesced.
//   mark    entry-parallel over the selected rows' stored entries (one contiguous span of colval): presence flag of every
//           kept local column in a bitmap over [j0, j1).  Coalesced reads; byte stores of the same value, no atomics.
//   scan    the library's three-phase scan (scan.h), twice: counts -> new rowptr (+ index_base), bitmap -> column look-up
//           table and the new col_indices.
//   fill    a workgroup per FILL_ROWS consecutive output rows: its writes are one contiguous run of the output, its reads
//           a few contiguous runs of the source.  Each lane owns FILL_V consecutive output entries and stores them with
//           16-byte accesses where the output is aligned (Guideline 13); colval' = lut[colval - j0].
//   values  the fill without the column half: refreshes the values of an earlier extraction from its per-row source starts
//           and its rowptr (16 bytes per row of map, against 8 per ENTRY for a source list fed to hpcla_gather_*, and the
//           same coalesced run structure as the fill).
//   column  one lane per row, one lower-bound search: out[i] = the stored value of column jk, else +0.0.
#include "common.h"
#include "scan.h"
#include "store16.h"

namespace hpcla {

constexpr int FILL_T = 256;        // threads per workgroup of the fill
constexpr int FILL_ROWS = 256;     // consecutive output rows per workgroup
constexpr int FILL_V = 4;          // consecutive output entries per lane: 16 bytes of 4-byte items, 2 x 16 of 8-byte items

template <typename I>
__device__ __forceinline__ int64_t lower_bound_col(const I *__restrict__ colval, int64_t a, int64_t b, int64_t key)
{
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if ((int64_t)colval[m] < key) a = m + 1; else b = m;
    }
    return a;
}

template <typename I>
__global__ __launch_bounds__(256) void submatrix_locate_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                               int64_t r0, int64_t nsel, int64_t j0, int64_t j1, int base,
                                                               int64_t *__restrict__ src_start, int64_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nsel) return;
    const int64_t a = (int64_t)rowptr[r0 + i] - base, b = (int64_t)rowptr[r0 + i + 1] - base;
    const int64_t lo = lower_bound_col(colval, a, b, j0 + base);
    const int64_t hi = lower_bound_col(colval, lo, b, j1 + base);
    src_start[i] = lo;
    cnt[i] = hi - lo;
}

template <typename I>
__global__ __launch_bounds__(256) void submatrix_mark_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                             int64_t nnz, int64_t r0, int64_t r1, int64_t j0, int64_t j1,
                                                             int base, unsigned char *__restrict__ present)
{
    const int64_t p0 = (int64_t)rowptr[r0] - base;
    int64_t p1 = (int64_t)rowptr[r1] - base;
    if (p1 > nnz) p1 = nnz;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t p = p0 + (int64_t)blockIdx.x * 256 + threadIdx.x; p < p1; p += stride) {
        const int64_t c = (int64_t)colval[p] - base;
        if (c >= j0 && c < j1) present[c - j0] = 1;
    }
}

// scan functors (scan.h).  Row counts are scanned over nsel + 1 elements, the last one worth 0: its emit writes rowptr'[nsel]
struct CountLoad {
    const int64_t *cnt;
    int64_t nsel;
    __device__ int64_t operator()(int64_t i) const { return i < nsel ? cnt[i] : 0; }
};
template <typename I>
struct RowptrEmit {
    I *rowptr_out;
    int base;
    __device__ void operator()(int64_t i, int64_t before, int64_t) const { rowptr_out[i] = (I)(before + base); }
};
struct ColumnLoad {
    const unsigned char *present;
    __device__ int64_t operator()(int64_t i) const { return present[i] ? 1 : 0; }
};
struct ColumnEmit {                       // lut[i] = rank of local column j0 + i among the kept ones; a kept one names itself
    int64_t j0;
    const int64_t *col_indices_src;       // global ids of the source's local columns, or null: emit the local column
    int64_t col_shift;
    int64_t *lut;
    int64_t *col_indices_out;
    __device__ void operator()(int64_t i, int64_t before, int64_t present) const
    {
        lut[i] = before;
        if (present) col_indices_out[before] = col_indices_src ? col_indices_src[j0 + i] - col_shift : j0 + i;
    }
};

// Output entry e of output row i reads source entry src_start[i] + (e - rowptr'[i]).  COLS: also colval' = lut[colval - j0].
template <typename I, typename E, bool COLS>
__global__ __launch_bounds__(FILL_T) void submatrix_fill_kernel(const I *__restrict__ colval, const E *__restrict__ nzval,
                                                                int64_t nnz_src, const int64_t *__restrict__ src_start,
                                                                const I *__restrict__ rowptr_out, int64_t nsel, int64_t nnz_out,
                                                                const int64_t *__restrict__ lut, int64_t j0, int64_t width,
                                                                int base, I *__restrict__ colval_out, E *__restrict__ nzval_out,
                                                                int aligned16)
{
    __shared__ int64_t s_rp[FILL_ROWS + 1];
    __shared__ int64_t s_src[FILL_ROWS];
    const int64_t b0 = (int64_t)blockIdx.x * FILL_ROWS;
    const int nb = (int)(nsel - b0 < FILL_ROWS ? nsel - b0 : FILL_ROWS);
    for (int t = threadIdx.x; t <= nb; t += FILL_T) {
        s_rp[t] = (int64_t)rowptr_out[b0 + t] - base;
        if (t < nb) s_src[t] = src_start[b0 + t];
    }
    __syncthreads();
    const int64_t e0 = s_rp[0];
    const int64_t e1 = s_rp[nb] < nnz_out ? s_rp[nb] : nnz_out;
    for (int64_t g = (e0 & ~(int64_t)(FILL_V - 1)) + (int64_t)threadIdx.x * FILL_V; g < e1; g += (int64_t)FILL_T * FILL_V) {
        const int64_t lo = g > e0 ? g : e0;
        const int64_t hi = g + FILL_V < e1 ? g + FILL_V : e1;
        if (lo >= hi) continue;
        int a = 0, b = nb;                               // the last row t with rowptr'[t] <= lo: empty rows before it are skipped
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (s_rp[m] <= lo) a = m; else b = m;
        }
        int t = a;
        E vals[FILL_V];
        I cols[FILL_V];
#pragma unroll
        for (int k = 0; k < FILL_V; ++k) {
            const int64_t e = g + k;
            vals[k] = 0;
            cols[k] = 0;
            if (e >= lo && e < hi) {
                while (e >= s_rp[t + 1]) ++t;            // e < e1 <= rowptr'[nb]: stops at t < nb
                const int64_t p = s_src[t] + (e - s_rp[t]);
                if (p >= 0 && p < nnz_src) {
                    vals[k] = nzval[p];
                    if (COLS) {
                        const int64_t c = (int64_t)colval[p] - base - j0;
                        if (c >= 0 && c < width) cols[k] = (I)(lut[c] + base);
                    }
                }
            }
        }
        if (aligned16 && lo == g && hi == g + FILL_V) {
            store_run(nzval_out + g, vals);
            if (COLS) store_run(colval_out + g, cols);
        } else {
#pragma unroll
            for (int k = 0; k < FILL_V; ++k) {
                const int64_t e = g + k;
                if (e >= lo && e < hi) {
                    nzval_out[e] = vals[k];
                    if (COLS) colval_out[e] = cols[k];
                }
            }
        }
    }
}

template <typename I, typename E>
__global__ __launch_bounds__(256) void sparse_column_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                            const E *__restrict__ nzval, int64_t nrows, int64_t nnz, int64_t jk,
                                                            int base, E *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    const int64_t a = (int64_t)rowptr[i] - base, b = (int64_t)rowptr[i + 1] - base;
    const int64_t p = lower_bound_col(colval, a, b, jk + base);
    E v = 0;                                             // all bits clear: +0.0
    if (p < b && p < nnz && (int64_t)colval[p] == jk + base) v = nzval[p];
    out[i] = v;
}

// main diagonal: one lane per local row i, a lower-bound search over the row's entries for the GLOBAL column row_start + i
// (col_indices is sorted and compressed columns ascend within a row, so col_indices[colval[.]] ascends too); the stored
// value bit for bit -- or its reciprocal -- and +0.0 (1 / +0.0 = inf) where nothing is stored
template <typename I>
__global__ __launch_bounds__(256) void sparse_diag_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                          const double *__restrict__ nzval, int64_t nrows, int64_t nnz, int base,
                                                          const int64_t *__restrict__ col_indices, int64_t ncomp,
                                                          int64_t row_start, int reciprocal, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    const int64_t key = row_start + i;
    int64_t a = (int64_t)rowptr[i] - base, b = (int64_t)rowptr[i + 1] - base;
    if (a < 0) a = 0;
    if (b > nnz) b = nnz;
    const int64_t end = b;
    auto global_col = [&](int64_t m) -> int64_t {
        const int64_t c = (int64_t)colval[m] - base;
        return (c >= 0 && c < ncomp) ? col_indices[c] : INT64_MAX;    // an id outside the table sorts last, is never read
    };
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (global_col(m) < key) a = m + 1; else b = m;
    }
    double v = 0.0;
    if (a < end && global_col(a) == key) v = nzval[a];
    out[i] = reciprocal ? 1.0 / v : v;
}

// work buffer: presence bitmap (width bytes, padded to 16) | lut (width words) | counts (nsel) | block sums of the two scans |
// the two totals
static int64_t work_bytes_of(int64_t nsel, int64_t width)
{
    return ((width + 15) / 16) * 16 + 8 * (width + nsel + scan_blocks(nsel + 1) + scan_blocks(width)) + 64;
}

struct WorkLayout {
    unsigned char *present;
    int64_t *lut, *cnt, *row_sums, *col_sums, *total;
    WorkLayout(void *work, int64_t nsel, int64_t width)
    {
        const int64_t pad = ((width + 15) / 16) * 16;
        present = reinterpret_cast<unsigned char *>(work);
        lut = reinterpret_cast<int64_t *>(present + pad);
        cnt = lut + width;
        row_sums = cnt + nsel;
        col_sums = row_sums + scan_blocks(nsel + 1);
        total = col_sums + scan_blocks(width);
    }
};

static int check_window(const char *what, int64_t nrows, int64_t nnz, int64_t r0, int64_t r1, int64_t j0, int64_t j1, int base)
{
    if (nrows < 0 || nnz < 0) return set_error(HPCLA_ERR_INVALID, "%s: negative size", what);
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "%s: index_base must be 0 or 1", what);
    if (r0 < 0 || r1 < r0 || r1 > nrows) return set_error(HPCLA_ERR_INVALID, "%s: row window outside [0, nrows]", what);
    if (j0 < 0 || j1 < j0) return set_error(HPCLA_ERR_INVALID, "%s: column window needs 0 <= j0 <= j1", what);
    return HPCLA_OK;
}

template <typename I>
static int structure_impl(const I *rowptr, const I *colval, int64_t nrows, int64_t nnz, int64_t r0, int64_t r1, int64_t j0,
                          int64_t j1, int base, const int64_t *col_indices_src, int64_t col_shift, int64_t *src_start,
                          I *rowptr_out, int64_t *col_indices_out, int64_t *nnz_out_host, int64_t *ncols_out_host, void *work,
                          void *stream)
{
    if (int rc = check_window("submatrix_structure", nrows, nnz, r0, r1, j0, j1, base)) return rc;
    const int64_t nsel = r1 - r0, width = j1 - j0;
    if (!rowptr || !rowptr_out || !work || !nnz_out_host || !ncols_out_host)
        return set_error(HPCLA_ERR_INVALID, "submatrix_structure: null rowptr / output / work");
    if ((nnz > 0 && !colval) || (nsel > 0 && !src_start) || (width > 0 && !col_indices_out))
        return set_error(HPCLA_ERR_INVALID, "submatrix_structure: null array with a non-zero size");
    hipStream_t s = as_stream(stream);
    WorkLayout w(work, nsel, width);
    HPCLA_CHECK_HIP(hipMemsetAsync(w.total, 0, 16, s));
    if (nsel > 0) {
        HPCLA_CHECK_GRID((nsel + 255) / 256, "submatrix_structure");
        submatrix_locate_kernel<I><<<(uint32_t)((nsel + 255) / 256), 256, 0, s>>>(rowptr, colval, r0, nsel, j0, j1, base,
                                                                                 src_start, w.cnt);
        HPCLA_CHECK_LAUNCH();
    }
    if (int rc = exclusive_scan(CountLoad{w.cnt, nsel}, nsel + 1, RowptrEmit<I>{rowptr_out, base}, w.row_sums, w.total, s))
        return rc;
    if (width > 0) {
        HPCLA_CHECK_HIP(hipMemsetAsync(w.present, 0, width, s));
        if (nsel > 0 && nnz > 0) {
            int64_t g = (nnz + 255) / 256;
            if (g > 4096) g = 4096;
            submatrix_mark_kernel<I><<<(uint32_t)g, 256, 0, s>>>(rowptr, colval, nnz, r0, r1, j0, j1, base, w.present);
            HPCLA_CHECK_LAUNCH();
        }
        if (int rc = exclusive_scan(ColumnLoad{w.present}, width, ColumnEmit{j0, col_indices_src, col_shift, w.lut, col_indices_out},
                                    w.col_sums, w.total + 1, s))
            return rc;
    }
    int64_t h[2] = {0, 0};
    HPCLA_CHECK_HIP(hipMemcpyAsync(h, w.total, 16, hipMemcpyDeviceToHost, s));
    HPCLA_CHECK_HIP(hipStreamSynchronize(s));            // the one synchronisation: the sizes the caller allocates by
    *nnz_out_host = h[0];
    *ncols_out_host = h[1];
    return HPCLA_OK;
}

template <typename I, typename E, bool COLS>
static int fill_launch(const I *colval, const void *nzval, int64_t nnz_src, const int64_t *src_start, const I *rowptr_out,
                       int64_t nsel, int64_t nnz_out, const int64_t *lut, int64_t j0, int64_t width, int base, I *colval_out,
                       void *nzval_out, hipStream_t s)
{
    const int64_t nblk = (nsel + FILL_ROWS - 1) / FILL_ROWS;
    HPCLA_CHECK_GRID(nblk, "submatrix fill");
    const int aligned16 = ((uintptr_t)nzval_out % 16 == 0) && (!COLS || (uintptr_t)colval_out % 16 == 0);
    submatrix_fill_kernel<I, E, COLS><<<(uint32_t)nblk, FILL_T, 0, s>>>(colval, static_cast<const E *>(nzval), nnz_src, src_start,
                                                                       rowptr_out, nsel, nnz_out, lut, j0, width, base,
                                                                       colval_out, static_cast<E *>(nzval_out), aligned16);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <typename I>
static int fill_impl(int elem_bytes, const I *colval, const void *nzval, int64_t nnz_src, const int64_t *src_start,
                     const I *rowptr_out, int64_t nsel, int64_t nnz_out, int64_t j0, int64_t j1, int base, const void *work,
                     I *colval_out, void *nzval_out, void *stream)
{
    if (elem_bytes != 4 && elem_bytes != 8) return set_error(HPCLA_ERR_INVALID, "submatrix_fill: elem_bytes must be 4 or 8");
    if (nnz_src < 0 || nsel < 0 || nnz_out < 0 || nnz_out > nnz_src)
        return set_error(HPCLA_ERR_INVALID, "submatrix_fill: bad sizes (need 0 <= nnz_out <= nnz_src, nsel >= 0)");
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "submatrix_fill: index_base must be 0 or 1");
    if (j0 < 0 || j1 < j0) return set_error(HPCLA_ERR_INVALID, "submatrix_fill: column window needs 0 <= j0 <= j1");
    if (nsel == 0 || nnz_out == 0) return HPCLA_OK;
    if (!colval || !nzval || !src_start || !rowptr_out || !work || !colval_out || !nzval_out)
        return set_error(HPCLA_ERR_INVALID, "submatrix_fill: null array with a non-zero size");
    WorkLayout w(const_cast<void *>(work), nsel, j1 - j0);
    hipStream_t s = as_stream(stream);
    return elem_bytes == 8
               ? fill_launch<I, uint64_t, true>(colval, nzval, nnz_src, src_start, rowptr_out, nsel, nnz_out, w.lut, j0, j1 - j0,
                                                base, colval_out, nzval_out, s)
               : fill_launch<I, uint32_t, true>(colval, nzval, nnz_src, src_start, rowptr_out, nsel, nnz_out, w.lut, j0, j1 - j0,
                                                base, colval_out, nzval_out, s);
}

template <typename I>
static int values_impl(int elem_bytes, const void *nzval, int64_t nnz_src, const int64_t *src_start, const I *rowptr_out,
                       int64_t nsel, int64_t nnz_out, int base, void *nzval_out, void *stream)
{
    if (elem_bytes != 4 && elem_bytes != 8) return set_error(HPCLA_ERR_INVALID, "submatrix_values: elem_bytes must be 4 or 8");
    if (nnz_src < 0 || nsel < 0 || nnz_out < 0 || nnz_out > nnz_src)
        return set_error(HPCLA_ERR_INVALID, "submatrix_values: bad sizes (need 0 <= nnz_out <= nnz_src, nsel >= 0)");
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "submatrix_values: index_base must be 0 or 1");
    if (nsel == 0 || nnz_out == 0) return HPCLA_OK;
    if (!nzval || !src_start || !rowptr_out || !nzval_out)
        return set_error(HPCLA_ERR_INVALID, "submatrix_values: null array with a non-zero size");
    hipStream_t s = as_stream(stream);
    return elem_bytes == 8 ? fill_launch<I, uint64_t, false>(nullptr, nzval, nnz_src, src_start, rowptr_out, nsel, nnz_out, nullptr,
                                                             0, 0, base, nullptr, nzval_out, s)
                           : fill_launch<I, uint32_t, false>(nullptr, nzval, nnz_src, src_start, rowptr_out, nsel, nnz_out, nullptr,
                                                             0, 0, base, nullptr, nzval_out, s);
}

template <typename I>
static int column_impl(int elem_bytes, const I *rowptr, const I *colval, const void *nzval, int64_t nrows, int64_t nnz,
                       int64_t jk, int base, void *out, void *stream)
{
    if (elem_bytes != 4 && elem_bytes != 8) return set_error(HPCLA_ERR_INVALID, "sparse_column: elem_bytes must be 4 or 8");
    if (nrows < 0 || nnz < 0 || jk < 0) return set_error(HPCLA_ERR_INVALID, "sparse_column: negative size or column");
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "sparse_column: index_base must be 0 or 1");
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr || !out || (nnz > 0 && (!colval || !nzval)))
        return set_error(HPCLA_ERR_INVALID, "sparse_column: null array with a non-zero size");
    HPCLA_CHECK_GRID((nrows + 255) / 256, "sparse_column");
    const uint32_t g = (uint32_t)((nrows + 255) / 256);
    hipStream_t s = as_stream(stream);
    if (elem_bytes == 8)
        sparse_column_kernel<I, uint64_t><<<g, 256, 0, s>>>(rowptr, colval, static_cast<const uint64_t *>(nzval), nrows, nnz, jk,
                                                           base, static_cast<uint64_t *>(out));
    else
        sparse_column_kernel<I, uint32_t><<<g, 256, 0, s>>>(rowptr, colval, static_cast<const uint32_t *>(nzval), nrows, nnz, jk,
                                                           base, static_cast<uint32_t *>(out));
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <typename I>
static int diag_impl(const I *rowptr, const I *colval, const double *nzval, int64_t nrows, int64_t nnz, int base,
                     const int64_t *col_indices, int64_t ncomp, int64_t row_start, int reciprocal, double *out, void *stream)
{
    if (nrows < 0 || nnz < 0 || ncomp < 0 || row_start < 0) return set_error(HPCLA_ERR_INVALID, "sparse_diag: negative size or row_start");
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "sparse_diag: index_base must be 0 or 1");
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr || !out || (nnz > 0 && (!colval || !nzval || !col_indices)))
        return set_error(HPCLA_ERR_INVALID, "sparse_diag: null array with a non-zero size");
    HPCLA_CHECK_GRID((nrows + 255) / 256, "sparse_diag");
    sparse_diag_kernel<I><<<(uint32_t)((nrows + 255) / 256), 256, 0, as_stream(stream)>>>(rowptr, colval, nzval, nrows, nnz, base,
                                                                                         col_indices, ncomp, row_start,
                                                                                         reciprocal, out);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_submatrix_scan_chunk(void) { return SCAN_B; }

HPCLA_API int64_t hpcla_submatrix_work_bytes(int64_t nsel, int64_t width)
{
    if (nsel < 0 || width < 0) return -1;
    return work_bytes_of(nsel, width);
}

HPCLA_API int hpcla_submatrix_structure_i32(const int32_t *rowptr, const int32_t *colval, int64_t nrows, int64_t nnz, int64_t r0,
                                            int64_t r1, int64_t j0, int64_t j1, int index_base, const int64_t *col_indices_src,
                                            int64_t col_shift, int64_t *src_start_out, int32_t *rowptr_out,
                                            int64_t *col_indices_out, int64_t *nnz_out_host, int64_t *ncols_out_host, void *work,
                                            void *stream)
{
    return structure_impl<int32_t>(rowptr, colval, nrows, nnz, r0, r1, j0, j1, index_base, col_indices_src, col_shift,
                                   src_start_out, rowptr_out, col_indices_out, nnz_out_host, ncols_out_host, work, stream);
}
HPCLA_API int hpcla_submatrix_structure_i64(const int64_t *rowptr, const int64_t *colval, int64_t nrows, int64_t nnz, int64_t r0,
                                            int64_t r1, int64_t j0, int64_t j1, int index_base, const int64_t *col_indices_src,
                                            int64_t col_shift, int64_t *src_start_out, int64_t *rowptr_out,
                                            int64_t *col_indices_out, int64_t *nnz_out_host, int64_t *ncols_out_host, void *work,
                                            void *stream)
{
    return structure_impl<int64_t>(rowptr, colval, nrows, nnz, r0, r1, j0, j1, index_base, col_indices_src, col_shift,
                                   src_start_out, rowptr_out, col_indices_out, nnz_out_host, ncols_out_host, work, stream);
}

HPCLA_API int hpcla_submatrix_fill_i32(int elem_bytes, const int32_t *colval, const void *nzval, int64_t nnz_src,
                                       const int64_t *src_start, const int32_t *rowptr_out, int64_t nsel, int64_t nnz_out,
                                       int64_t j0, int64_t j1, int index_base, const void *work, int32_t *colval_out,
                                       void *nzval_out, void *stream)
{
    return fill_impl<int32_t>(elem_bytes, colval, nzval, nnz_src, src_start, rowptr_out, nsel, nnz_out, j0, j1, index_base, work,
                              colval_out, nzval_out, stream);
}
HPCLA_API int hpcla_submatrix_fill_i64(int elem_bytes, const int64_t *colval, const void *nzval, int64_t nnz_src,
                                       const int64_t *src_start, const int64_t *rowptr_out, int64_t nsel, int64_t nnz_out,
                                       int64_t j0, int64_t j1, int index_base, const void *work, int64_t *colval_out,
                                       void *nzval_out, void *stream)
{
    return fill_impl<int64_t>(elem_bytes, colval, nzval, nnz_src, src_start, rowptr_out, nsel, nnz_out, j0, j1, index_base, work,
                              colval_out, nzval_out, stream);
}

HPCLA_API int hpcla_submatrix_values_i32(int elem_bytes, const void *nzval, int64_t nnz_src, const int64_t *src_start,
                                         const int32_t *rowptr_out, int64_t nsel, int64_t nnz_out, int index_base,
                                         void *nzval_out, void *stream)
{
    return values_impl<int32_t>(elem_bytes, nzval, nnz_src, src_start, rowptr_out, nsel, nnz_out, index_base, nzval_out, stream);
}
HPCLA_API int hpcla_submatrix_values_i64(int elem_bytes, const void *nzval, int64_t nnz_src, const int64_t *src_start,
                                         const int64_t *rowptr_out, int64_t nsel, int64_t nnz_out, int index_base,
                                         void *nzval_out, void *stream)
{
    return values_impl<int64_t>(elem_bytes, nzval, nnz_src, src_start, rowptr_out, nsel, nnz_out, index_base, nzval_out, stream);
}

HPCLA_API int hpcla_sparse_column_i32(int elem_bytes, const int32_t *rowptr, const int32_t *colval, const void *nzval,
                                      int64_t nrows, int64_t nnz, int64_t jk, int index_base, void *out, void *stream)
{
    return column_impl<int32_t>(elem_bytes, rowptr, colval, nzval, nrows, nnz, jk, index_base, out, stream);
}
HPCLA_API int hpcla_sparse_column_i64(int elem_bytes, const int64_t *rowptr, const int64_t *colval, const void *nzval,
                                      int64_t nrows, int64_t nnz, int64_t jk, int index_base, void *out, void *stream)
{
    return column_impl<int64_t>(elem_bytes, rowptr, colval, nzval, nrows, nnz, jk, index_base, out, stream);
}

HPCLA_API int hpcla_sparse_diag_f64_i32(const int32_t *rowptr, const int32_t *colval, const double *nzval, int64_t nrows,
                                        int64_t nnz, int index_base, const int64_t *col_indices, int64_t n_col_indices,
                                        int64_t row_start, int reciprocal, double *out, void *stream)
{
    return diag_impl<int32_t>(rowptr, colval, nzval, nrows, nnz, index_base, col_indices, n_col_indices, row_start, reciprocal,
                              out, stream);
}
HPCLA_API int hpcla_sparse_diag_f64_i64(const int64_t *rowptr, const int64_t *colval, const double *nzval, int64_t nrows,
                                        int64_t nnz, int index_base, const int64_t *col_indices, int64_t n_col_indices,
                                        int64_t row_start, int reciprocal, double *out, void *stream)
{
    return diag_impl<int64_t>(rowptr, colval, nzval, nrows, nnz, index_base, col_indices, n_col_indices, row_start, reciprocal,
                              out, stream);
}
