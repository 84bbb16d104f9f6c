// select.hip -- index-set selection on the device: A[rows, cols] for index LISTS, v[idx] and v[idx] = src.
//
// Reference (host, entry by entry): Base.getindex(A::HPCSparseMatrix, row_idx::HPCVector{Int}, col_idx::HPCVector{Int})
// gathers col_idx to every rank, builds a Dict from column to position and walks every selected row through it
// (src/indexing.jl:1654-1815, extract_sparse_row :1743-1765); it returns a DENSE HPCMatrix (:1640-1644), which is unusable at
// the sizes this library works at: here the result is an HPCSparseMatrix, as range indexing gives (submatrix.hip).
// Base.getindex(v, idx::HPCVector{Int}) (:1339-1460) and Base.setindex!(v, src, idx) (:1871-1985) are the vector forms.
//
// The range form is a copy, because a row keeps one contiguous run of its entries.  This one is not: kept entries lie
// scattered through the row, and after a column permutation they must be put in ascending order of their NEW column to keep
// the struct's invariant (columns ascend within a row).  New columns are distinct within a row (the
// caller refuses duplicated columns), so the place of a kept entry is rowptr'[r] + the number of kept entries of its row
// with a smaller new column: a rank, found by comparing integers; nothing is sorted and no atomics are used.  Values are
// moved, never computed with: the kernels are templated on the element SIZE and copy integers.
//
// Passes (all on the caller's stream):
//   look-up  one lane per compressed column of A: lower-bound search of its global id in the caller's sorted column list;
//            the column's new global position, or -1.
//   count    SEL_G lanes per selected row stream the row's entries: the kept count of every output row, a presence flag of
//            every new column that occurs (byte stores of the same value), the longest kept row per workgroup.
//   scan     the library's scan (scan.h), twice: counts -> new rowptr, bitmap -> the result's col_indices and, composed with
//            the look-up, the table from A's compressed column to the result's compressed column (-1: dropped).
//   fill     rank and fill, in three forms by KEPT row length n:
//              n <= SEL_SHORT_CAP  SEL_G lanes per row, SEL_ROWS consecutive output rows per workgroup;
//              n <= SEL_TILE       a workgroup per row, the kept entries of the row in LDS;
//              n >  SEL_TILE       a workgroup per row: every tile of SEL_TILE kept entries is ranked against the whole row,
//                                  streamed through LDS once per tile -- QUADRATIC in the row length; the slow case, correct.
//            The host launches the two long forms only when the longest kept row (read back with the sizes) needs them.
//            Reads are a gather by nature under a permutation (cdna_hip_programming.md, Guideline 2 and Appendix B
//            "Scatter / gather"); the writes of a workgroup of the first two forms are ONE contiguous run of the output,
//            staged in LDS and stored in whole 16-byte accesses where aligned (Guideline 13).  The third form scatters
//            within its row's run.
//   values   out[p] = nzval2[src[p]] with the int64 source positions the fill recorded: hpcla_gather_f64_i64 for 8-byte
//            elements, hpcla_gather_b32_i64 (here) for 4-byte ones.
//   take/put out[i] = pos[i] < n_own ? v[pos[i]] : ghost[pos[i] - n_own];  v[pos[i]] = src[i].
#include <limits>

#include "common.h"
#include "scan.h"
#include "store16.h"

namespace hpcla {

constexpr int SEL_T = 256;                       // threads per workgroup
constexpr int SEL_G = 8;                         // lanes per row: count pass and short fill
constexpr int SEL_ROWS = SEL_T / SEL_G;          // 32 consecutive output rows per workgroup
constexpr int SEL_SHORT_CAP = 32;                // kept entries of a row of the short form
constexpr int SEL_TILE = 1024;                   // kept entries of a row held in LDS
constexpr int SEL_V = 4;                         // consecutive output entries per lane of a staged store
constexpr int64_t SEL_NONE = INT64_MAX;          // a new column that sorts last: padding of an LDS slot

static inline int64_t sel_count_blocks(int64_t nsel) { return (nsel + SEL_ROWS - 1) / SEL_ROWS; }

__global__ __launch_bounds__(256) void select_lookup_kernel(const int64_t *__restrict__ col_indices_src, int64_t ncomp,
                                                            const int64_t *__restrict__ sorted_cols,
                                                            const int64_t *__restrict__ sorted_pos, int64_t nsorted,
                                                            int listed, int64_t width, int base,
                                                            int64_t *__restrict__ newcol)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ncomp) return;
    const int64_t key = col_indices_src[j];
    int64_t pos = -1;
    if (!listed) {
        pos = key - base;                        // all columns, in order
    } else {
        int64_t a = 0, b = nsorted;
        while (a < b) {
            const int64_t m = a + ((b - a) >> 1);
            if (sorted_cols[m] < key) a = m + 1; else b = m;
        }
        if (a < nsorted && sorted_cols[a] == key) pos = sorted_pos[a];
    }
    newcol[j] = (pos >= 0 && pos < width) ? pos : -1;
}

// the stored entries [a, b) of selected row i (empty for a row outside the matrix)
template <typename I>
__device__ __forceinline__ void row_span(const I *__restrict__ rowptr, const int64_t *__restrict__ rows, int64_t i, int64_t nrows,
                                         int64_t nnz, int base, int64_t &a, int64_t &b)
{
    const int64_t r = rows ? rows[i] : i;
    a = b = 0;
    if (r < 0 || r >= nrows) return;
    a = (int64_t)rowptr[r] - base;
    b = (int64_t)rowptr[r + 1] - base;
    if (a < 0) a = 0;
    if (b > nnz) b = nnz;
    if (b < a) b = a;
}

// the result's compressed column of source entry p, or -1
template <typename I>
__device__ __forceinline__ int64_t mapped_col(const I *__restrict__ colval, const int64_t *__restrict__ table, int64_t ncomp,
                                              int base, int64_t p)
{
    const int64_t j = (int64_t)colval[p] - base;
    return (j >= 0 && j < ncomp) ? table[j] : -1;
}

template <typename I>
__global__ __launch_bounds__(SEL_T) void select_count_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                             int64_t nrows, int64_t nnz, int64_t ncomp,
                                                             const int64_t *__restrict__ rows, int64_t nsel,
                                                             const int64_t *__restrict__ newcol, int base,
                                                             int64_t *__restrict__ cnt, unsigned char *__restrict__ present,
                                                             int64_t *__restrict__ block_max)
{
    __shared__ int64_t s_n[SEL_ROWS];
    const int g = threadIdx.x / SEL_G, sub = threadIdx.x % SEL_G;
    const int64_t i = (int64_t)blockIdx.x * SEL_ROWS + g;
    int64_t n = 0;
    if (i < nsel) {
        int64_t a, b;
        row_span(rowptr, rows, i, nrows, nnz, base, a, b);
        for (int64_t p = a + sub; p < b; p += SEL_G) {
            const int64_t c = mapped_col(colval, newcol, ncomp, base, p);
            if (c >= 0) {
                ++n;
                present[c] = 1;
            }
        }
    }
#pragma unroll
    for (int off = SEL_G / 2; off > 0; off >>= 1) n += __shfl_xor(n, off, SEL_G);
    if (sub == 0) {
        s_n[g] = n;
        if (i < nsel) cnt[i] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t m = 0;
        for (int k = 0; k < SEL_ROWS; ++k) m = s_n[k] > m ? s_n[k] : m;
        block_max[blockIdx.x] = m;
    }
}

// one workgroup: total[2] = the largest of block_max[0 .. nb)
static __global__ __launch_bounds__(SEL_T) void select_max_kernel(const int64_t *__restrict__ block_max, int64_t nb,
                                                                  int64_t *__restrict__ total)
{
    __shared__ int64_t s_m[SEL_T];
    int64_t m = 0;
    for (int64_t k = threadIdx.x; k < nb; k += SEL_T) m = block_max[k] > m ? block_max[k] : m;
    s_m[threadIdx.x] = m;
    __syncthreads();
    for (int off = SEL_T / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off && s_m[threadIdx.x + off] > s_m[threadIdx.x]) s_m[threadIdx.x] = s_m[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[2] = s_m[0];
}

// scan functors (scan.h).  Row counts are scanned over nsel + 1 elements, the last one worth 0: its emit writes rowptr'[nsel]
struct SelCountLoad {
    const int64_t *cnt;
    int64_t nsel;
    __device__ int64_t operator()(int64_t i) const { return i < nsel ? cnt[i] : 0; }
};
template <typename I>
struct SelRowptrEmit {
    I *rowptr_out;
    int base;
    __device__ void operator()(int64_t i, int64_t before, int64_t) const { rowptr_out[i] = (I)(before + base); }
};
struct SelColumnLoad {
    const unsigned char *present;
    __device__ int64_t operator()(int64_t i) const { return present[i] ? 1 : 0; }
};
struct SelColumnEmit {                    // lut[c] = rank of new column c among those that occur; one that occurs names itself
    int64_t *lut;
    int64_t *col_indices_out;
    int base;
    __device__ void operator()(int64_t i, int64_t before, int64_t present) const
    {
        lut[i] = before;
        if (present) col_indices_out[before] = i + base;
    }
};

// table[j]: A's compressed column j -> new global position (in) -> the result's compressed column (out); -1 stays -1
__global__ __launch_bounds__(256) void select_compose_kernel(int64_t *__restrict__ table, int64_t ncomp,
                                                             const int64_t *__restrict__ lut, int64_t width)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= ncomp) return;
    const int64_t c = table[j];
    table[j] = (c >= 0 && c < width) ? lut[c] : -1;
}

// Output entries [e0, e0 + n) of a workgroup, staged in LDS in output order (new compressed column s_oc, source position s_op),
// leave in whole 16-byte accesses where the outputs are aligned; the values are gathered here.
template <typename I, typename E>
__device__ __forceinline__ void emit_run(int64_t e0, int64_t n, const int64_t *s_oc, const int64_t *s_op,
                                         const E *__restrict__ nzval, int64_t nnz, int base, I *__restrict__ colval_out,
                                         E *__restrict__ nzval_out, int64_t *__restrict__ src_out, int aligned16)
{
    const int64_t e1 = e0 + n;
    for (int64_t g = (e0 & ~(int64_t)(SEL_V - 1)) + (int64_t)threadIdx.x * SEL_V; g < e1; g += (int64_t)SEL_T * SEL_V) {
        const int64_t lo = g > e0 ? g : e0;
        const int64_t hi = g + SEL_V < e1 ? g + SEL_V : e1;
        if (lo >= hi) continue;
        E vals[SEL_V];
        I cols[SEL_V];
        int64_t src[SEL_V];
#pragma unroll
        for (int k = 0; k < SEL_V; ++k) {
            const int64_t e = g + k;
            vals[k] = 0;
            cols[k] = 0;
            src[k] = 0;
            if (e >= lo && e < hi) {
                const int64_t p = s_op[e - e0];
                src[k] = p;
                cols[k] = (I)(s_oc[e - e0] + base);
                if (p >= 0 && p < nnz) vals[k] = nzval[p];
            }
        }
        if (aligned16 && lo == g && hi == g + SEL_V) {
            store_run(nzval_out + g, vals);
            store_run(colval_out + g, cols);
            store_run(src_out + g, src);
        } else {
#pragma unroll
            for (int k = 0; k < SEL_V; ++k) {
                const int64_t e = g + k;
                if (e >= lo && e < hi) {
                    nzval_out[e] = vals[k];
                    colval_out[e] = cols[k];
                    src_out[e] = src[k];
                }
            }
        }
    }
}

// short rows: SEL_G lanes stream a row and compact its kept entries into the row's LDS slot (ballot within the lane group:
// the order is the stored one), rank them there, and place them into the workgroup's staged run
template <typename I, typename E>
__global__ __launch_bounds__(SEL_T) void select_fill_short_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                  const E *__restrict__ nzval, int64_t nrows, int64_t nnz,
                                                                  int64_t ncomp, const int64_t *__restrict__ rows, int64_t nsel,
                                                                  const I *__restrict__ rowptr_out, int64_t nnz_out,
                                                                  const int64_t *__restrict__ table, int base,
                                                                  I *__restrict__ colval_out, E *__restrict__ nzval_out,
                                                                  int64_t *__restrict__ src_out, int aligned16)
{
    __shared__ int64_t s_rp[SEL_ROWS + 1];
    __shared__ int s_off[SEL_ROWS + 1];
    __shared__ int s_all_short;
    __shared__ int64_t s_c[SEL_ROWS * SEL_SHORT_CAP], s_p[SEL_ROWS * SEL_SHORT_CAP];
    __shared__ int64_t s_oc[SEL_ROWS * SEL_SHORT_CAP], s_op[SEL_ROWS * SEL_SHORT_CAP];
    const int64_t b0 = (int64_t)blockIdx.x * SEL_ROWS;
    const int nb = (int)(nsel - b0 < SEL_ROWS ? nsel - b0 : SEL_ROWS);
    for (int t = threadIdx.x; t <= nb; t += SEL_T) {
        int64_t e = (int64_t)rowptr_out[b0 + t] - base;
        s_rp[t] = e < 0 ? 0 : (e > nnz_out ? nnz_out : e);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int off = 0, all_short = 1;
        for (int t = 0; t < nb; ++t) {
            const int64_t len = s_rp[t + 1] - s_rp[t];
            s_off[t] = off;
            if (len > SEL_SHORT_CAP) all_short = 0;
            else if (len > 0) off += (int)len;
        }
        s_off[nb] = off;
        s_all_short = all_short;
    }
    __syncthreads();
    const int g = threadIdx.x / SEL_G, sub = threadIdx.x % SEL_G;
    const int lane = threadIdx.x & 63;
    const int64_t len64 = g < nb ? s_rp[g + 1] - s_rp[g] : 0;
    const int len = (len64 > 0 && len64 <= SEL_SHORT_CAP) ? (int)len64 : 0;       // 0: nothing to do here, or a longer form's row
    int64_t *row_c = s_c + g * SEL_SHORT_CAP, *row_p = s_p + g * SEL_SHORT_CAP;
    if (len > 0) {
        int64_t a, b;
        row_span(rowptr, rows, b0 + g, nrows, nnz, base, a, b);
        int have = 0;
        for (int64_t p0 = a; p0 < b && have < len; p0 += SEL_G) {                 // uniform within the lane group
            const int64_t p = p0 + sub;
            const int64_t c = p < b ? mapped_col(colval, table, ncomp, base, p) : -1;
            const unsigned mask = (unsigned)(__ballot(c >= 0) >> (lane & ~(SEL_G - 1))) & ((1u << SEL_G) - 1);
            const int slot = have + __popc(mask & ((1u << sub) - 1));
            if (c >= 0 && slot < len) {
                row_c[slot] = c;
                row_p[slot] = p;
            }
            have += __popc(mask);
        }
        for (int q = have + sub; q < len; q += SEL_G) {                           // counts and rows disagree: defined padding
            row_c[q] = SEL_NONE;
            row_p[q] = -1;
        }
    }
    __syncthreads();
    if (len > 0) {
        const int off = s_off[g];
        for (int q = sub; q < len; q += SEL_G) {
            const int64_t c = row_c[q];
            int rank = 0;
            for (int j = 0; j < len; ++j) rank += row_c[j] < c;
            s_oc[off + rank] = c;
            s_op[off + rank] = row_p[q];
        }
    }
    __syncthreads();
    int total = s_off[nb];
    if (s_rp[0] + total > nnz_out) total = (int)(nnz_out - s_rp[0]);
    if (s_all_short) {                           // the staged entries are the run [rowptr'[b0], rowptr'[b0 + nb])
        emit_run(s_rp[0], (int64_t)total, s_oc, s_op, nzval, nnz, base, colval_out, nzval_out, src_out, aligned16);
    } else {                                     // a longer row lies between them: entry by entry
        for (int q = threadIdx.x; q < total; q += SEL_T) {
            int a = 0, b = nb;                   // the last row t with s_off[t] <= q that holds staged entries
            while (b - a > 1) {
                const int m = (a + b) >> 1;
                if (s_off[m] <= q) a = m; else b = m;
            }
            const int64_t e = s_rp[a] + (q - s_off[a]);
            const int64_t p = s_op[q];
            if (e < nnz_out) {
                colval_out[e] = (I)(s_oc[q] + base);
                nzval_out[e] = (p >= 0 && p < nnz) ? nzval[p] : (E)0;
                src_out[e] = p;
            }
        }
    }
}

// A workgroup streams the stored entries [a, b) of a row; the kept ones are numbered in stored order (ballot per wave, the
// waves' counts through LDS), and those numbered [k_lo, k_hi) land in s_c / s_p at their number - k_lo.  Ends on a barrier.
template <typename I>
__device__ __forceinline__ int64_t collect_kept(const I *__restrict__ colval, const int64_t *__restrict__ table, int64_t ncomp,
                                                int base, int64_t a, int64_t b, int64_t k_lo, int64_t k_hi, int64_t *s_c,
                                                int64_t *s_p, int *s_w)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t have = 0;
    for (int64_t p0 = a; p0 < b && have < k_hi; p0 += SEL_T) {                    // uniform over the workgroup
        const int64_t p = p0 + threadIdx.x;
        const int64_t c = p < b ? mapped_col(colval, table, ncomp, base, p) : -1;
        const unsigned long long mask = __ballot(c >= 0);
        if (lane == 0) s_w[w] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < SEL_T / 64; ++k) {
            if (k < w) before += s_w[k];
            all += s_w[k];
        }
        const int64_t k = have + before + __popcll(mask & ((1ull << lane) - 1));
        if (c >= 0 && k >= k_lo && k < k_hi) {
            s_c[k - k_lo] = c;
            s_p[k - k_lo] = p;
        }
        have += all;
        __syncthreads();
    }
    for (int64_t q = (have > k_lo ? have : k_lo) + threadIdx.x; q < k_hi; q += SEL_T) {       // defined padding
        s_c[q - k_lo] = SEL_NONE;
        s_p[q - k_lo] = -1;
    }
    __syncthreads();
    return have;
}

// rows of SEL_SHORT_CAP < n <= SEL_TILE kept entries: a workgroup per row (grid-stride over the selected rows)
template <typename I, typename E>
__global__ __launch_bounds__(SEL_T) void select_fill_tile_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                 const E *__restrict__ nzval, int64_t nrows, int64_t nnz,
                                                                 int64_t ncomp, const int64_t *__restrict__ rows, int64_t nsel,
                                                                 const I *__restrict__ rowptr_out, int64_t nnz_out,
                                                                 const int64_t *__restrict__ table, int base,
                                                                 I *__restrict__ colval_out, E *__restrict__ nzval_out,
                                                                 int64_t *__restrict__ src_out, int aligned16)
{
    __shared__ int64_t s_c[SEL_TILE], s_p[SEL_TILE], s_oc[SEL_TILE], s_op[SEL_TILE];
    __shared__ int s_w[SEL_T / 64];
    for (int64_t i = blockIdx.x; i < nsel; i += gridDim.x) {
        const int64_t e0 = (int64_t)rowptr_out[i] - base;
        const int64_t len = (int64_t)rowptr_out[i + 1] - base - e0;
        if (len <= SEL_SHORT_CAP || len > SEL_TILE || e0 < 0 || e0 + len > nnz_out) continue;
        int64_t a, b;
        row_span(rowptr, rows, i, nrows, nnz, base, a, b);
        collect_kept(colval, table, ncomp, base, a, b, 0, len, s_c, s_p, s_w);
        for (int q = threadIdx.x; q < (int)len; q += SEL_T) {
            const int64_t c = s_c[q];
            int rank = 0;
            for (int j = 0; j < (int)len; ++j) rank += s_c[j] < c;
            s_oc[rank] = c;
            s_op[rank] = s_p[q];
        }
        __syncthreads();
        emit_run(e0, len, s_oc, s_op, nzval, nnz, base, colval_out, nzval_out, src_out, aligned16);
        __syncthreads();
    }
}

// rows of more than SEL_TILE kept entries: every tile of kept entries is ranked against the whole row, which is streamed
// through LDS once per tile -- quadratic, the slow case.  The entries of a tile scatter over the row's run of the output.
template <typename I, typename E>
__global__ __launch_bounds__(SEL_T) void select_fill_long_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                 const E *__restrict__ nzval, int64_t nrows, int64_t nnz,
                                                                 int64_t ncomp, const int64_t *__restrict__ rows, int64_t nsel,
                                                                 const I *__restrict__ rowptr_out, int64_t nnz_out,
                                                                 const int64_t *__restrict__ table, int base,
                                                                 I *__restrict__ colval_out, E *__restrict__ nzval_out,
                                                                 int64_t *__restrict__ src_out)
{
    constexpr int PER = SEL_TILE / SEL_T;
    __shared__ int64_t s_c[SEL_TILE], s_p[SEL_TILE], s_b[SEL_T];
    __shared__ int s_w[SEL_T / 64];
    for (int64_t i = blockIdx.x; i < nsel; i += gridDim.x) {
        const int64_t e0 = (int64_t)rowptr_out[i] - base;
        const int64_t len = (int64_t)rowptr_out[i + 1] - base - e0;
        if (len <= SEL_TILE || e0 < 0 || e0 + len > nnz_out) continue;
        int64_t a, b;
        row_span(rowptr, rows, i, nrows, nnz, base, a, b);
        for (int64_t k_lo = 0; k_lo < len; k_lo += SEL_TILE) {
            const int64_t k_hi = k_lo + SEL_TILE < len ? k_lo + SEL_TILE : len;
            const int na = (int)(k_hi - k_lo);
            collect_kept(colval, table, ncomp, base, a, b, k_lo, k_hi, s_c, s_p, s_w);
            int64_t mine[PER], rank[PER];
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int q = threadIdx.x + u * SEL_T;
                mine[u] = q < na ? s_c[q] : SEL_NONE;
                rank[u] = 0;
            }
            for (int64_t p0 = a; p0 < b; p0 += SEL_T) {
                const int64_t p = p0 + threadIdx.x;
                const int64_t c = p < b ? mapped_col(colval, table, ncomp, base, p) : -1;
                s_b[threadIdx.x] = c >= 0 ? c : SEL_NONE;              // a dropped entry is smaller than nothing
                __syncthreads();
                for (int j = 0; j < SEL_T; ++j) {
                    const int64_t v = s_b[j];
#pragma unroll
                    for (int u = 0; u < PER; ++u) rank[u] += v < mine[u];
                }
                __syncthreads();
            }
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int q = threadIdx.x + u * SEL_T;
                if (q < na && mine[u] != SEL_NONE && rank[u] < len) {
                    const int64_t e = e0 + rank[u];
                    const int64_t p = s_p[q];
                    colval_out[e] = (I)(mine[u] + base);
                    nzval_out[e] = (p >= 0 && p < nnz) ? nzval[p] : (E)0;
                    src_out[e] = p;
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void gather_b32_kernel(const uint32_t *__restrict__ x, const int64_t *__restrict__ src,
                                                         uint32_t *__restrict__ out, int64_t n, int64_t nx, int base)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t p = src[i] - base;
        out[i] = (p >= 0 && p < nx) ? x[p] : 0u;
    }
}

template <typename P>
__global__ __launch_bounds__(256) void take_kernel(const double *__restrict__ v, int64_t n_own, const double *__restrict__ ghost,
                                                   int64_t n_ghost, const P *__restrict__ pos, int64_t n, int base,
                                                   double *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t p = (int64_t)pos[i] - base;
        double x = 0.0;
        if (p >= 0 && p < n_own) x = v[p];
        else if (p >= n_own && p - n_own < n_ghost) x = ghost[p - n_own];
        out[i] = x;
    }
}

template <typename P>
__global__ __launch_bounds__(256) void put_kernel(double *__restrict__ v, int64_t n_own, const P *__restrict__ pos,
                                                  const double *__restrict__ src, int64_t n, int base)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t p = (int64_t)pos[i] - base;
        if (p >= 0 && p < n_own) v[p] = src[i];
    }
}

static uint32_t stream_blocks(int64_t n)
{
    const int64_t g = (n + 255) / 256;
    return (uint32_t)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// work buffer, 8-byte words first: table (ncomp) | lut (width) | counts (nsel) | the count pass's block maxima | block sums of
// the two scans | the three totals | presence bitmap (width bytes).  `fill` reads the table alone, which therefore comes first.
static int64_t work_bytes_of(int64_t nsel, int64_t ncomp, int64_t width)
{
    return 8 * (ncomp + width + nsel + sel_count_blocks(nsel) + scan_blocks(nsel + 1) + scan_blocks(width) + 8)
           + ((width + 15) / 16) * 16;
}

struct SelWork {
    int64_t *table, *lut, *cnt, *block_max, *row_sums, *col_sums, *total;
    unsigned char *present;
    SelWork(void *work, int64_t nsel, int64_t ncomp, int64_t width)
    {
        table = reinterpret_cast<int64_t *>(work);
        lut = table + ncomp;
        cnt = lut + width;
        block_max = cnt + nsel;
        row_sums = block_max + sel_count_blocks(nsel);
        col_sums = row_sums + scan_blocks(nsel + 1);
        total = col_sums + scan_blocks(width);
        present = reinterpret_cast<unsigned char *>(total + 8);
    }
};

template <typename I>
static int structure_impl(const I *rowptr, const I *colval, int64_t nrows, int64_t nnz, const int64_t *col_indices_src,
                          int64_t ncomp, const int64_t *rows, int64_t nsel, const int64_t *sorted_cols,
                          const int64_t *sorted_pos, int64_t nsorted, int64_t width, int base, I *rowptr_out,
                          int64_t *col_indices_out, int64_t *nnz_out_host, int64_t *ncols_out_host, int64_t *max_row_host,
                          void *work, void *stream)
{
    if (nrows < 0 || nnz < 0 || ncomp < 0 || nsel < 0 || nsorted < -1 || width < 0)
        return set_error(HPCLA_ERR_INVALID, "select_structure: negative size");
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "select_structure: index_base must be 0 or 1");
    if (!rowptr || !rowptr_out || !work || !nnz_out_host || !ncols_out_host || !max_row_host)
        return set_error(HPCLA_ERR_INVALID, "select_structure: null rowptr / output / work");
    if (nsorted > 0 && (!sorted_cols || !sorted_pos))
        return set_error(HPCLA_ERR_INVALID, "select_structure: null sorted_cols / sorted_pos with a non-zero size");
    if ((nnz > 0 && !colval) || (ncomp > 0 && !col_indices_src) || (width > 0 && ncomp > 0 && !col_indices_out))
        return set_error(HPCLA_ERR_INVALID, "select_structure: null array with a non-zero size");
    hipStream_t s = as_stream(stream);
    SelWork w(work, nsel, ncomp, width);
    HPCLA_CHECK_HIP(hipMemsetAsync(w.total, 0, 64, s));
    if (ncomp > 0) {
        HPCLA_CHECK_GRID((ncomp + 255) / 256, "select_structure");
        select_lookup_kernel<<<(uint32_t)((ncomp + 255) / 256), 256, 0, s>>>(col_indices_src, ncomp, sorted_cols, sorted_pos,
                                                                            nsorted < 0 ? 0 : nsorted, nsorted >= 0, width, base,
                                                                            w.table);
        HPCLA_CHECK_LAUNCH();
    }
    if (width > 0) HPCLA_CHECK_HIP(hipMemsetAsync(w.present, 0, width, s));
    if (nsel > 0) {
        const int64_t nb = sel_count_blocks(nsel);
        HPCLA_CHECK_GRID(nb, "select_structure");
        select_count_kernel<I><<<(uint32_t)nb, SEL_T, 0, s>>>(rowptr, colval, nrows, nnz, ncomp, rows, nsel, w.table, base, w.cnt,
                                                             w.present, w.block_max);
        HPCLA_CHECK_LAUNCH();
        select_max_kernel<<<1, SEL_T, 0, s>>>(w.block_max, nb, w.total);
        HPCLA_CHECK_LAUNCH();
    }
    if (int rc = exclusive_scan(SelCountLoad{w.cnt, nsel}, nsel + 1, SelRowptrEmit<I>{rowptr_out, base}, w.row_sums, w.total, s))
        return rc;
    if (width > 0) {
        if (int rc = exclusive_scan(SelColumnLoad{w.present}, width, SelColumnEmit{w.lut, col_indices_out, base}, w.col_sums,
                                    w.total + 1, s))
            return rc;
        if (ncomp > 0) {
            select_compose_kernel<<<(uint32_t)((ncomp + 255) / 256), 256, 0, s>>>(w.table, ncomp, w.lut, width);
            HPCLA_CHECK_LAUNCH();
        }
    }
    int64_t h[3] = {0, 0, 0};
    HPCLA_CHECK_HIP(hipMemcpyAsync(h, w.total, 24, hipMemcpyDeviceToHost, s));
    HPCLA_CHECK_HIP(hipStreamSynchronize(s));            // the one synchronisation: the sizes the caller allocates by
    *nnz_out_host = h[0];
    *ncols_out_host = h[1];
    *max_row_host = h[2];
    if (h[0] + base > (int64_t)std::numeric_limits<I>::max())        // rowptr_out has wrapped: the caller must not use it
        return set_error(HPCLA_ERR_UNSUPPORTED, "select_structure: the result's %lld entries do not fit the index type",
                         (long long)h[0]);
    return HPCLA_OK;
}

template <typename I, typename E>
static int fill_launch(const I *rowptr, const I *colval, const void *nzval_v, int64_t nrows, int64_t nnz, int64_t ncomp,
                       const int64_t *rows, int64_t nsel, const I *rowptr_out, int64_t nnz_out, int64_t max_row, int base,
                       const int64_t *table, I *colval_out, void *nzval_out_v, int64_t *src_out, hipStream_t s)
{
    const E *nzval = static_cast<const E *>(nzval_v);
    E *nzval_out = static_cast<E *>(nzval_out_v);
    const int aligned16 = (uintptr_t)nzval_out % 16 == 0 && (uintptr_t)colval_out % 16 == 0 && (uintptr_t)src_out % 16 == 0;
    const int64_t nb = sel_count_blocks(nsel);
    HPCLA_CHECK_GRID(nb, "select_fill");
    select_fill_short_kernel<I, E><<<(uint32_t)nb, SEL_T, 0, s>>>(rowptr, colval, nzval, nrows, nnz, ncomp, rows, nsel, rowptr_out,
                                                                 nnz_out, table, base, colval_out, nzval_out, src_out, aligned16);
    HPCLA_CHECK_LAUNCH();
    const uint32_t grid = (uint32_t)(nsel < 4096 ? nsel : 4096);
    if (max_row < 0 || max_row > SEL_SHORT_CAP) {
        select_fill_tile_kernel<I, E><<<grid, SEL_T, 0, s>>>(rowptr, colval, nzval, nrows, nnz, ncomp, rows, nsel, rowptr_out,
                                                            nnz_out, table, base, colval_out, nzval_out, src_out, aligned16);
        HPCLA_CHECK_LAUNCH();
    }
    if (max_row < 0 || max_row > SEL_TILE) {
        select_fill_long_kernel<I, E><<<grid, SEL_T, 0, s>>>(rowptr, colval, nzval, nrows, nnz, ncomp, rows, nsel, rowptr_out,
                                                            nnz_out, table, base, colval_out, nzval_out, src_out);
        HPCLA_CHECK_LAUNCH();
    }
    return HPCLA_OK;
}

template <typename I>
static int fill_impl(int elem_bytes, const I *rowptr, const I *colval, const void *nzval, int64_t nrows, int64_t nnz,
                     int64_t ncomp, const int64_t *rows, int64_t nsel, const I *rowptr_out, int64_t nnz_out, int64_t max_row,
                     int base, const void *work, I *colval_out, void *nzval_out, int64_t *src_out, void *stream)
{
    if (elem_bytes != 4 && elem_bytes != 8) return set_error(HPCLA_ERR_INVALID, "select_fill: elem_bytes must be 4 or 8");
    if (nrows < 0 || nnz < 0 || ncomp < 0 || nsel < 0 || nnz_out < 0)
        return set_error(HPCLA_ERR_INVALID, "select_fill: negative size");
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "select_fill: index_base must be 0 or 1");
    if (nsel == 0 || nnz_out == 0) return HPCLA_OK;
    if (!rowptr || !colval || !nzval || !rowptr_out || !work || !colval_out || !nzval_out || !src_out)
        return set_error(HPCLA_ERR_INVALID, "select_fill: null array with a non-zero size");
    const int64_t *table = static_cast<const int64_t *>(work);
    hipStream_t s = as_stream(stream);
    return elem_bytes == 8 ? fill_launch<I, uint64_t>(rowptr, colval, nzval, nrows, nnz, ncomp, rows, nsel, rowptr_out, nnz_out,
                                                      max_row, base, table, colval_out, nzval_out, src_out, s)
                           : fill_launch<I, uint32_t>(rowptr, colval, nzval, nrows, nnz, ncomp, rows, nsel, rowptr_out, nnz_out,
                                                      max_row, base, table, colval_out, nzval_out, src_out, s);
}

template <typename P>
static int take_impl(const double *v, int64_t n_own, const double *ghost, int64_t n_ghost, const P *pos, int64_t n, int base,
                     double *out, void *stream)
{
    if (n_own < 0 || n_ghost < 0 || n < 0) return set_error(HPCLA_ERR_INVALID, "select_take: negative size");
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "select_take: index_base must be 0 or 1");
    if (n == 0) return HPCLA_OK;
    if (!pos || !out || (n_own > 0 && !v) || (n_ghost > 0 && !ghost))
        return set_error(HPCLA_ERR_INVALID, "select_take: null array with a non-zero size");
    take_kernel<P><<<stream_blocks(n), 256, 0, as_stream(stream)>>>(v, n_own, ghost, n_ghost, pos, n, base, out);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <typename P>
static int put_impl(double *v, int64_t n_own, const P *pos, const double *src, int64_t n, int base, void *stream)
{
    if (n_own < 0 || n < 0) return set_error(HPCLA_ERR_INVALID, "select_put: negative size");
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "select_put: index_base must be 0 or 1");
    if (n == 0 || n_own == 0) return HPCLA_OK;
    if (!v || !pos || !src) return set_error(HPCLA_ERR_INVALID, "select_put: null array with a non-zero size");
    put_kernel<P><<<stream_blocks(n), 256, 0, as_stream(stream)>>>(v, n_own, pos, src, n, base);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_select_short_cap(void) { return SEL_SHORT_CAP; }
HPCLA_API int64_t hpcla_select_tile(void) { return SEL_TILE; }

HPCLA_API int64_t hpcla_select_work_bytes(int64_t nsel, int64_t ncomp, int64_t width)
{
    if (nsel < 0 || ncomp < 0 || width < 0) return -1;
    return work_bytes_of(nsel, ncomp, width);
}

HPCLA_API int hpcla_select_structure_i32(const int32_t *rowptr, const int32_t *colval, int64_t nrows, int64_t nnz,
                                         const int64_t *col_indices_src, int64_t ncomp, const int64_t *rows, int64_t nsel,
                                         const int64_t *sorted_cols, const int64_t *sorted_pos, int64_t nsorted, int64_t width,
                                         int index_base, int32_t *rowptr_out, int64_t *col_indices_out, int64_t *nnz_out_host,
                                         int64_t *ncols_out_host, int64_t *max_row_host, void *work, void *stream)
{
    return structure_impl<int32_t>(rowptr, colval, nrows, nnz, col_indices_src, ncomp, rows, nsel, sorted_cols, sorted_pos, nsorted,
                                   width, index_base, rowptr_out, col_indices_out, nnz_out_host, ncols_out_host, max_row_host, work,
                                   stream);
}
HPCLA_API int hpcla_select_structure_i64(const int64_t *rowptr, const int64_t *colval, int64_t nrows, int64_t nnz,
                                         const int64_t *col_indices_src, int64_t ncomp, const int64_t *rows, int64_t nsel,
                                         const int64_t *sorted_cols, const int64_t *sorted_pos, int64_t nsorted, int64_t width,
                                         int index_base, int64_t *rowptr_out, int64_t *col_indices_out, int64_t *nnz_out_host,
                                         int64_t *ncols_out_host, int64_t *max_row_host, void *work, void *stream)
{
    return structure_impl<int64_t>(rowptr, colval, nrows, nnz, col_indices_src, ncomp, rows, nsel, sorted_cols, sorted_pos, nsorted,
                                   width, index_base, rowptr_out, col_indices_out, nnz_out_host, ncols_out_host, max_row_host, work,
                                   stream);
}

HPCLA_API int hpcla_select_fill_i32(int elem_bytes, const int32_t *rowptr, const int32_t *colval, const void *nzval, int64_t nrows,
                                    int64_t nnz, int64_t ncomp, const int64_t *rows, int64_t nsel, const int32_t *rowptr_out,
                                    int64_t nnz_out, int64_t max_row, int index_base, const void *work, int32_t *colval_out,
                                    void *nzval_out, int64_t *src_out, void *stream)
{
    return fill_impl<int32_t>(elem_bytes, rowptr, colval, nzval, nrows, nnz, ncomp, rows, nsel, rowptr_out, nnz_out, max_row,
                              index_base, work, colval_out, nzval_out, src_out, stream);
}
HPCLA_API int hpcla_select_fill_i64(int elem_bytes, const int64_t *rowptr, const int64_t *colval, const void *nzval, int64_t nrows,
                                    int64_t nnz, int64_t ncomp, const int64_t *rows, int64_t nsel, const int64_t *rowptr_out,
                                    int64_t nnz_out, int64_t max_row, int index_base, const void *work, int64_t *colval_out,
                                    void *nzval_out, int64_t *src_out, void *stream)
{
    return fill_impl<int64_t>(elem_bytes, rowptr, colval, nzval, nrows, nnz, ncomp, rows, nsel, rowptr_out, nnz_out, max_row,
                              index_base, work, colval_out, nzval_out, src_out, stream);
}

HPCLA_API int hpcla_gather_b32_i64(const void *x, const int64_t *src, void *out, int64_t n, int64_t nx, int index_base,
                                   void *stream)
{
    if (n < 0 || nx < 0) return set_error(HPCLA_ERR_INVALID, "gather_b32: negative size");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "gather_b32: index_base must be 0 or 1");
    if (n == 0) return HPCLA_OK;
    if (!src || !out || (nx > 0 && !x)) return set_error(HPCLA_ERR_INVALID, "gather_b32: null array with a non-zero size");
    gather_b32_kernel<<<stream_blocks(n), 256, 0, as_stream(stream)>>>(static_cast<const uint32_t *>(x), src,
                                                                      static_cast<uint32_t *>(out), n, nx, index_base);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_select_take_f64_i32(const double *v, int64_t n_own, const double *ghost, int64_t n_ghost, const int32_t *pos,
                                        int64_t n, int index_base, double *out, void *stream)
{
    return take_impl<int32_t>(v, n_own, ghost, n_ghost, pos, n, index_base, out, stream);
}
HPCLA_API int hpcla_select_take_f64_i64(const double *v, int64_t n_own, const double *ghost, int64_t n_ghost, const int64_t *pos,
                                        int64_t n, int index_base, double *out, void *stream)
{
    return take_impl<int64_t>(v, n_own, ghost, n_ghost, pos, n, index_base, out, stream);
}
HPCLA_API int hpcla_select_put_f64_i32(double *v, int64_t n_own, const int32_t *pos, const double *src, int64_t n, int index_base,
                                       void *stream)
{
    return put_impl<int32_t>(v, n_own, pos, src, n, index_base, stream);
}
HPCLA_API int hpcla_select_put_f64_i64(double *v, int64_t n_own, const int64_t *pos, const double *src, int64_t n, int index_base,
                                       void *stream)
{
    return put_impl<int64_t>(v, n_own, pos, src, n, index_base, stream);
}
