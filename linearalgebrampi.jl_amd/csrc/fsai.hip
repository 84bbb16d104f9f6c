// fsai.hip -- setup of the factorised sparse approximate inverse preconditioner (hp.fsai; Kolotilina-Yeremin): a sparse lower
// triangular G with G A G' ~ I on a given pattern, M = G' G.  Applying M is two SpMVs on ordinary plans; this file only builds G.
//
// Row i of G (local row of a rank, partitions of rows and columns agree, so a split column c < n_own IS local row c):
//   J_i   the columns c < i of pattern row i, ascending, then i itself (the diagonal is always part of the row); m = |J_i|.
//         Split columns >= n_own are ghosts and never < i <= n_own - 1, so "c < i" alone selects the owned lower part; a row in
//         split space is not sorted as a whole, its owned columns are ascending among themselves.
//   S     A[J_i, J_i], dense m x m; an entry A does not store is 0.  Only the lower triangle of S is read.
//   S = L L', row i of G on J_i = inv(L') e_m: one back-substitution.  diag(G A G') = 1.
//
// count   m per row through the shared three-phase scan (scan.h): G's rowptr, nnz(G), the largest m; a row with m > 32 or whose
//         diagonal A does not store is recorded in the error word.
// factor  groups of MT = 4, 8, 16 or 32 lanes serve one row (64 / MT rows per wave, MT from the largest m of the launch).  Lane c
//         of a group holds row c of S (the entries of row J_i[c] of A that hit J_i) in MT registers; the group is padded with
//         rows of the identity, which no operation below mixes into the first m rows, so the bits of a row do not depend on MT.
//         Every register array is indexed by compile-time constants only (fully unrolled loops): no scratch.
//           for k = 0 .. MT-1:  d = S[k][k] (from lane k);  !(d > 0): the row is not positive definite (NaN included)
//                               L[k][k] = sqrt(d);  L[c][k] = S[c][k] / L[k][k]  (c > k)
//                               for j = k+1 .. MT-1:  S[c][j] = S[c][j] - L[c][k] * L[j][k]     (L[j][k] from lane j)
//                               lane k keeps column k of L (the L[j][k] it has just seen): row k of L', in the unused upper
//                               part of its own row
//           acc = e_m;  for j = MT-1 .. 0:  y_j = acc_j / L[j][j] (lane j), acc_c = acc_c - L[j][c] * y_j  (c < j)
//         Products and sums are separately rounded (-ffp-contract=off); the order is fixed by the row alone.
//         The same kernel writes G's global column ids and values (the "fill": a row's m entries by its first m lanes).
// Error word (one device word, vector atomic min): (local row << 2) | code of the smallest failing row; all ones = none.
// No loop waits on another workgroup; the only atomics are that min and the max of m.
#include "common.h"
#include "scan.h"

namespace hpcla {

constexpr int FSAI_THREADS = 256;
constexpr int FSAI_MAX_M = 32;
constexpr unsigned long long FSAI_CAP = 1, FSAI_NO_DIAG = 2, FSAI_NOT_SPD = 3;

// m of row i: 1 + the stored pattern columns below i
template <typename I>
struct FsaiCountLoad {
    const I *p_rowptr, *p_colval;
    int base;
    __device__ int64_t operator()(int64_t i) const
    {
        const int64_t e0 = (int64_t)p_rowptr[i] - base, e1 = (int64_t)p_rowptr[i + 1] - base;
        int64_t m = 1;
        for (int64_t e = e0; e < e1; ++e) m += ((int64_t)p_colval[e] - base < i) ? 1 : 0;
        return m;
    }
};

template <typename I>
struct FsaiCountEmit {
    const I *a_rowptr, *a_colval;
    int base;
    int64_t nrows;
    int64_t *g_rowptr, *info;
    __device__ void operator()(int64_t i, int64_t before, int64_t m) const
    {
        g_rowptr[i] = before;
        if (i == nrows - 1) {
            g_rowptr[nrows] = before + m;
            info[0] = before + m;
        }
        if (m > info[1]) atomicMax(reinterpret_cast<long long *>(info + 1), (long long)m);
        unsigned long long *err = reinterpret_cast<unsigned long long *>(info + 2);
        if (m > FSAI_MAX_M) atomicMin(err, ((unsigned long long)i << 2) | FSAI_CAP);
        const int64_t e0 = (int64_t)a_rowptr[i] - base, e1 = (int64_t)a_rowptr[i + 1] - base;
        bool diag = false;
        for (int64_t e = e0; e < e1; ++e) diag = diag || ((int64_t)a_colval[e] - base == i);
        if (!diag) atomicMin(err, ((unsigned long long)i << 2) | FSAI_NO_DIAG);
    }
};

template <typename I, int MT>
__global__ __launch_bounds__(FSAI_THREADS) void fsai_factor_kernel(const I *__restrict__ p_rowptr, const I *__restrict__ p_colval,
                                                                   const I *__restrict__ a_rowptr, const I *__restrict__ a_colval,
                                                                   const double *__restrict__ a_nzval, int64_t nrows, int base,
                                                                   int64_t col_start, const int64_t *__restrict__ g_rowptr,
                                                                   int64_t *__restrict__ g_cols, double *__restrict__ g_vals,
                                                                   int64_t *__restrict__ info)
{
    const int64_t i = ((int64_t)blockIdx.x * FSAI_THREADS + threadIdx.x) / MT;
    const int c = threadIdx.x & (MT - 1);
    bool live = i < nrows;
    unsigned long long *err = reinterpret_cast<unsigned long long *>(info + 2);

    // J_i, whole, in every lane of the group (the lanes read the same addresses)
    I J[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) J[k] = -1;
    int m = 0;
    if (live) {
        const int64_t e0 = (int64_t)p_rowptr[i] - base, e1 = (int64_t)p_rowptr[i + 1] - base;
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t col = (int64_t)p_colval[e] - base;
            if (col < i) {
#pragma unroll
                for (int k = 0; k < MT; ++k)
                    if (m == k) J[k] = (I)col;
                ++m;
            }
        }
#pragma unroll
        for (int k = 0; k < MT; ++k)
            if (m == k) J[k] = (I)i;
        ++m;
        if (m > MT) {                                        // a caller's max_m below the truth: recorded, nothing written
            if (c == 0) atomicMin(err, ((unsigned long long)i << 2) | FSAI_CAP);
            live = false;
        }
    }
    if (!live) {
        m = 0;
#pragma unroll
        for (int k = 0; k < MT; ++k) J[k] = -1;
    }
    int64_t jmine = -1;
#pragma unroll
    for (int k = 0; k < MT; ++k)
        if (k == c) jmine = J[k];

    // row c of S; lanes c >= m hold a row of the identity
    double s[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) s[k] = (k == c && c >= m) ? 1.0 : 0.0;
    if (c < m) {
        const int64_t e0 = (int64_t)a_rowptr[jmine] - base, e1 = (int64_t)a_rowptr[jmine + 1] - base;
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t col = (int64_t)a_colval[e] - base;
            const double v = a_nzval[e];
#pragma unroll
            for (int k = 0; k < MT; ++k)
                if (col == (int64_t)J[k]) s[k] = v;
        }
    }

    // S = L L' across the group's lanes.  Lane k keeps column k of L (the L[j][k] it has just seen, j > k: row k of L') in the
    // upper part of its own row, which nothing reads as S.
    double dmine = 1.0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < MT; ++k) {
        const double dk = __shfl(s[k], k, MT);
        if (!(dk > 0.0)) bad = true;
        const double lkk = sqrt(dk);
        const double lk = (c == k) ? lkk : s[k] / lkk;
        s[k] = c >= k ? lk : s[k];                          // lanes c < k hold L[k][c] there
        if (c == k) dmine = lkk;
#pragma unroll
        for (int j = k + 1; j < MT; ++j) {
            const double ljk = __shfl(lk, j, MT);
            const double upd = s[j] - lk * ljk;
            s[j] = c > k ? upd : (c == k ? ljk : s[j]);
        }
    }

    // L' y = e_m
    double acc = (c == m - 1) ? 1.0 : 0.0, y = 0.0;
#pragma unroll
    for (int j = MT - 1; j >= 0; --j) {
        const double yj = __shfl(acc / dmine, j, MT);
        if (c == j) y = yj;
        if (c < j) acc = acc - s[j] * yj;
    }

    if (live) {
        if (c < m) {
            const int64_t pos = g_rowptr[i] + c;
            g_cols[pos] = col_start + jmine;
            g_vals[pos] = bad ? 0.0 : y;
        }
        if (bad && c == 0) atomicMin(err, ((unsigned long long)i << 2) | FSAI_NOT_SPD);
    }
}

template <typename I>
static int fsai_count_impl(const I *p_rowptr, const I *p_colval, const I *a_rowptr, const I *a_colval, int64_t nrows,
                           int64_t n_own, int index_base, int64_t *g_rowptr, int64_t *info, void *work, void *stream)
{
    if (nrows < 0 || n_own != nrows) return set_error(HPCLA_ERR_INVALID, "fsai_count: needs n_own == nrows >= 0");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "fsai_count: index_base must be 0 or 1");
    if (!g_rowptr || !info || !work) return set_error(HPCLA_ERR_INVALID, "fsai_count: null rowptr / info / work");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(info, 0, 2 * sizeof(int64_t), s));
    HPCLA_CHECK_HIP(hipMemsetAsync(info + 2, 0xff, sizeof(int64_t), s));
    if (nrows == 0) {
        HPCLA_CHECK_HIP(hipMemsetAsync(g_rowptr, 0, sizeof(int64_t), s));
        return HPCLA_OK;
    }
    if (!p_rowptr || !p_colval || !a_rowptr || !a_colval) return set_error(HPCLA_ERR_INVALID, "fsai_count: null CSR array");
    int64_t *sums = reinterpret_cast<int64_t *>(work);
    return exclusive_scan(FsaiCountLoad<I>{p_rowptr, p_colval, index_base},
                          nrows, FsaiCountEmit<I>{a_rowptr, a_colval, index_base, nrows, g_rowptr, info}, sums + 1, sums, s);
}

template <typename I>
static int fsai_factor_impl(const I *p_rowptr, const I *p_colval, const I *a_rowptr, const I *a_colval, const double *a_nzval,
                            int64_t nrows, int64_t n_own, int index_base, int64_t col_start, int max_m, const int64_t *g_rowptr,
                            int64_t *g_cols, double *g_vals, int64_t *info, void *stream)
{
    if (nrows < 0 || n_own != nrows) return set_error(HPCLA_ERR_INVALID, "fsai_factor: needs n_own == nrows >= 0");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "fsai_factor: index_base must be 0 or 1");
    if (max_m < 1 || max_m > FSAI_MAX_M) return set_error(HPCLA_ERR_INVALID, "fsai_factor: needs 1 <= max_m <= 32");
    if (!info) return set_error(HPCLA_ERR_INVALID, "fsai_factor: null info");
    if (nrows == 0) return HPCLA_OK;
    if (!p_rowptr || !p_colval || !a_rowptr || !a_colval || !a_nzval || !g_rowptr || !g_cols || !g_vals)
        return set_error(HPCLA_ERR_INVALID, "fsai_factor: null array");
    const int mt = max_m <= 4 ? 4 : (max_m <= 8 ? 8 : (max_m <= 16 ? 16 : 32));
    const int64_t nb = (nrows * mt + FSAI_THREADS - 1) / FSAI_THREADS;
    HPCLA_CHECK_GRID(nb, "fsai_factor");
    hipStream_t s = as_stream(stream);
#define HPCLA_FSAI_FACTOR(MT)                                                                                              \
    fsai_factor_kernel<I, MT><<<(uint32_t)nb, FSAI_THREADS, 0, s>>>(p_rowptr, p_colval, a_rowptr, a_colval, a_nzval, nrows, \
                                                                    index_base, col_start, g_rowptr, g_cols, g_vals, info)
    switch (mt) {
    case 4: HPCLA_FSAI_FACTOR(4); break;
    case 8: HPCLA_FSAI_FACTOR(8); break;
    case 16: HPCLA_FSAI_FACTOR(16); break;
    default: HPCLA_FSAI_FACTOR(32); break;
    }
#undef HPCLA_FSAI_FACTOR
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_fsai_work_bytes(int64_t nrows)
{
    if (nrows < 0) return -1;
    return (int64_t)sizeof(int64_t) * (1 + scan_blocks(nrows > 0 ? nrows : 1));
}

HPCLA_API int hpcla_fsai_count_f64_i32(const int32_t *p_rowptr, const int32_t *p_colval_split, const int32_t *a_rowptr,
                                       const int32_t *a_colval_split, int64_t nrows, int64_t n_own, int index_base,
                                       int64_t *g_rowptr_dev, int64_t *info_dev, void *work, void *stream)
{
    return fsai_count_impl<int32_t>(p_rowptr, p_colval_split, a_rowptr, a_colval_split, nrows, n_own, index_base, g_rowptr_dev,
                                    info_dev, work, stream);
}

HPCLA_API int hpcla_fsai_count_f64_i64(const int64_t *p_rowptr, const int64_t *p_colval_split, const int64_t *a_rowptr,
                                       const int64_t *a_colval_split, int64_t nrows, int64_t n_own, int index_base,
                                       int64_t *g_rowptr_dev, int64_t *info_dev, void *work, void *stream)
{
    return fsai_count_impl<int64_t>(p_rowptr, p_colval_split, a_rowptr, a_colval_split, nrows, n_own, index_base, g_rowptr_dev,
                                    info_dev, work, stream);
}

HPCLA_API int hpcla_fsai_factor_f64_i32(const int32_t *p_rowptr, const int32_t *p_colval_split, const int32_t *a_rowptr,
                                        const int32_t *a_colval_split, const double *a_nzval, int64_t nrows, int64_t n_own,
                                        int index_base, int64_t col_start, int max_m, const int64_t *g_rowptr_dev,
                                        int64_t *g_cols_dev, double *g_vals_dev, int64_t *info_dev, void *stream)
{
    return fsai_factor_impl<int32_t>(p_rowptr, p_colval_split, a_rowptr, a_colval_split, a_nzval, nrows, n_own, index_base,
                                     col_start, max_m, g_rowptr_dev, g_cols_dev, g_vals_dev, info_dev, stream);
}

HPCLA_API int hpcla_fsai_factor_f64_i64(const int64_t *p_rowptr, const int64_t *p_colval_split, const int64_t *a_rowptr,
                                        const int64_t *a_colval_split, const double *a_nzval, int64_t nrows, int64_t n_own,
                                        int index_base, int64_t col_start, int max_m, const int64_t *g_rowptr_dev,
                                        int64_t *g_cols_dev, double *g_vals_dev, int64_t *info_dev, void *stream)
{
    return fsai_factor_impl<int64_t>(p_rowptr, p_colval_split, a_rowptr, a_colval_split, a_nzval, nrows, n_own, index_base,
                                     col_start, max_m, g_rowptr_dev, g_cols_dev, g_vals_dev, info_dev, stream);
}
