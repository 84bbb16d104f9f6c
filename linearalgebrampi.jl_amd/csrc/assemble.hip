// assemble.hip -- COO assembly on the device: sparse(I, J, V, m, n) with a structure that is built once and values that are
// summed again at every step (hp.assembly_plan).
//
// Reference: the users' idiom is Julia's sparse(I, J, V, m, n) on the host followed by HPCSparseMatrix(A, backend)
// (src/sparse.jl:398-413); a finite-element loop repeats both, and the upload, for every new V on the same (I, J).
//
// Here the structure is an inverted index (cdna_hip_programming.md Appendix B, "Scatter / gather / embedding": a sum per
// destination through the list of its contributions, no atomics).  A stable sort of the keys (row - row_lo) * ncols + col
// gives `perm`; the positions where the sorted key changes give `seg_ptr`; output entry e sums the values at
// perm[seg_ptr[e] .. seg_ptr[e + 1]), which ascend because the sort is stable.
//
// Sum order (it fixes the bits).  CH = ASM_CH.  A segment of L <= CH contributions is one chain s = v[p1]; s = s + v[p2]; ...
// left to right, started from the first value and not from 0.0 (a lone -0.0 stays -0.0).  A longer one is cut into
// consecutive chunks of CH contributions, each summed by that rule, and the partial sums are added left to right in chunk
// order.  Only adds occur.
//
// Plan-time passes (once per structure, all on the caller's stream):
//   keys       one lane per triplet: the key, and the count and first position of indices outside the matrix and of rows
//              outside [row_lo, row_hi) (integer atomics on four words).
//   segments   the library's scan (scan.h) over the head flags of the sorted keys: seg_ptr and the unique keys.
//   row_starts one lane per row, a lower-bound search: rowptr over the unique keys, or -- the vector form -- seg_ptr over the
//              sorted keys themselves, where rows without a contribution are empty segments.
//   columns    unique key -> global column.
// Assembly-time passes (the hot path; no synchronisation, no read-back):
//   values     a workgroup owns ASM_RUN consecutive output entries, so its part of the sorted list is one contiguous span.
//              It walks the span in passes of ASM_PASS contributions: every lane reads ASM_PASS / ASM_T entries of perm
//              (coalesced), issues all its gathers before the first lands in LDS, and then one lane per segment adds its
//              values from LDS in list order.  A segment that crosses a pass goes on from its accumulator in LDS, so the
//              chain is the same wherever the passes cut it.  Accumulators start at +0.0, which is what an empty segment
//              of the vector form stores.  The run's sums leave with one coalesced store per lane and entry.
//   long       only when a segment may be longer than CH: a wave per tile of CH list positions finds, with two searches in
//              seg_ptr, the at most two chunks of long segments that START in its tile, sums each from LDS in order and
//              stores the partial sum in a slot of its own.  `values` skips the span of a long segment and adds its
//              partial sums in chunk order instead: a hub entry costs its workgroup one add per chunk, the chunks run on
//              as many waves as there are.
#include "common.h"
#include "scan.h"

namespace hpcla {

constexpr int ASM_T = 256;                      // threads per workgroup of the values pass
constexpr int ASM_RUN = 1024;                   // consecutive output entries per workgroup
constexpr int ASM_PASS = 2048;                  // contributions staged in LDS per pass
constexpr int ASM_K = ASM_PASS / ASM_T;         // gathers in flight per lane
constexpr int ASM_CH = 512;                     // chunk of the sum order
constexpr int ASM_CK = ASM_CH / 64;             // gathers in flight per lane of a chunk's wave

__global__ __launch_bounds__(256) void assemble_keys_kernel(const int64_t *__restrict__ rows, const int64_t *__restrict__ cols,
                                                            int64_t n, int64_t row_lo, int64_t row_hi, int64_t nrows_global,
                                                            int64_t ncols, int base, int64_t *__restrict__ key,
                                                            unsigned long long *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = rows[i] - base;
    const int64_t c = cols ? cols[i] - base : 0;
    int64_t k = INT64_MAX;                                            // a refused triplet sorts last; the plan raises anyway
    if (r < 0 || r >= nrows_global || c < 0 || c >= ncols) {
        atomicAdd(&counts[0], 1ull);
        atomicMin(&counts[1], (unsigned long long)i);
    } else if (r < row_lo || r >= row_hi) {
        atomicAdd(&counts[2], 1ull);
        atomicMin(&counts[3], (unsigned long long)i);
    } else {
        k = (r - row_lo) * ncols + c;
    }
    key[i] = k;
}

struct HeadLoad {
    const int64_t *skey;
    __device__ int64_t operator()(int64_t i) const { return (i == 0 || skey[i] != skey[i - 1]) ? 1 : 0; }
};
template <typename S>
struct HeadEmit {                         // segment `before` starts at i; the element after the last closes seg_ptr
    const int64_t *skey;
    int64_t n;
    S *seg_ptr;
    int64_t *ukey;
    __device__ void operator()(int64_t i, int64_t before, int64_t head) const
    {
        if (head) {
            seg_ptr[before] = (S)i;
            ukey[before] = skey[i];
        }
        if (i == n - 1) seg_ptr[before + head] = (S)n;
    }
};

// out[r] = the first position whose key is >= r * ncols, r in [0, nrows]
template <typename O>
__global__ __launch_bounds__(256) void assemble_row_starts_kernel(const int64_t *__restrict__ keys, int64_t n, int64_t nrows,
                                                                  int64_t ncols, int base, O *__restrict__ out)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r > nrows) return;
    int64_t a = 0, b = n;
    if (r == nrows) {
        a = n;                                                        // r * ncols may not be representable
    } else {
        const int64_t want = r * ncols;
        while (a < b) {
            const int64_t m = a + ((b - a) >> 1);
            if (keys[m] < want) a = m + 1; else b = m;
        }
    }
    out[r] = (O)(a + base);
}

__global__ __launch_bounds__(256) void assemble_columns_kernel(const int64_t *__restrict__ ukey, int64_t nnz, int64_t ncols,
                                                               int base, int64_t *__restrict__ colidx)
{
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= nnz) return;
    const int64_t k = ukey[u];
    colidx[u] = k - (k / ncols) * ncols + base;
}

// value p of the rank's list [vals | ghost]; a position outside both reads as +0.0 and nothing is touched
__device__ __forceinline__ double list_value(int64_t p, const double *__restrict__ vals, int64_t n_own,
                                             const double *__restrict__ ghost, int64_t n_ghost)
{
    if (p < 0) return 0.0;
    if (p < n_own) return vals[p];
    if (p - n_own < n_ghost) return ghost[p - n_own];
    return 0.0;
}

__device__ __forceinline__ int64_t clamp_pos(int64_t v, int64_t n) { return v < 0 ? 0 : (v > n ? n : v); }

// slot of the partial sum of chunk c of a long segment that starts at s0: two slots per tile of CH list positions, the odd
// one for a segment's first chunk (at most one segment starts a chunk 0 in a tile and goes on past its end; at most one other
// chunk, of the segment that holds the tile's first position, starts in it)
__device__ __forceinline__ int64_t partial_slot(int64_t s0, int64_t c)
{
    return 2 * ((s0 + c * ASM_CH) / ASM_CH) + (c == 0 ? 1 : 0);
}

template <typename S>
__global__ __launch_bounds__(64) void assemble_long_kernel(const S *__restrict__ seg_ptr, const S *__restrict__ perm,
                                                           int64_t nseg, int64_t n_in, const double *__restrict__ vals,
                                                           int64_t n_own, const double *__restrict__ ghost, int64_t n_ghost,
                                                           double *__restrict__ partials)
{
    __shared__ double s_val[ASM_CH];
    const int lane = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * ASM_CH;
    const int64_t t1 = t0 + ASM_CH < n_in ? t0 + ASM_CH : n_in;
    int64_t cand[2];
    for (int q = 0; q < 2; ++q) {                                     // the segments holding the tile's first and last position
        const int64_t pos = q == 0 ? t0 : t1 - 1;
        int64_t a = 0, b = nseg;                                      // last a with seg_ptr[a] <= pos
        while (b - a > 1) {
            const int64_t m = a + ((b - a) >> 1);
            if (clamp_pos((int64_t)seg_ptr[m], n_in) <= pos) a = m; else b = m;
        }
        cand[q] = a;
    }
    for (int q = 0; q < 2; ++q) {
        if (q == 1 && cand[1] == cand[0]) break;
        const int64_t u = cand[q];
        const int64_t s0 = clamp_pos((int64_t)seg_ptr[u], n_in), s1 = clamp_pos((int64_t)seg_ptr[u + 1], n_in);
        if (s1 - s0 <= ASM_CH) continue;
        const int64_t c = s0 < t0 ? (t0 - s0 + ASM_CH - 1) / ASM_CH : 0;
        const int64_t p = s0 + c * ASM_CH;                            // the chunk of u that starts at or after t0
        if (p < t0 || p >= t1 || p >= s1) continue;
        const int64_t pe = p + ASM_CH < s1 ? p + ASM_CH : s1;
        int64_t idx[ASM_CK];
#pragma unroll
        for (int k = 0; k < ASM_CK; ++k) {
            const int64_t i = p + lane + k * 64;
            idx[k] = i < pe ? (int64_t)perm[i] : -1;
        }
        double v[ASM_CK];
#pragma unroll
        for (int k = 0; k < ASM_CK; ++k) v[k] = list_value(idx[k], vals, n_own, ghost, n_ghost);
        __syncthreads();                                              // the previous candidate's chain has read s_val
#pragma unroll
        for (int k = 0; k < ASM_CK; ++k) s_val[lane + k * 64] = v[k];
        __syncthreads();
        if (lane == 0) {
            const int len = (int)(pe - p);
            double s = s_val[0];
            for (int j = 1; j < len; ++j) s = s + s_val[j];
            partials[partial_slot(s0, c)] = s;
        }
    }
}

template <typename S>
__global__ __launch_bounds__(ASM_T) void assemble_values_kernel(const S *__restrict__ seg_ptr, const S *__restrict__ perm,
                                                                int64_t nseg, int64_t n_in, const double *__restrict__ vals,
                                                                int64_t n_own, const double *__restrict__ ghost,
                                                                int64_t n_ghost, const double *__restrict__ partials,
                                                                double *__restrict__ out)
{
    __shared__ int64_t s_ptr[ASM_RUN + 1];
    __shared__ double s_acc[ASM_RUN];
    __shared__ double s_val[ASM_PASS];
    const int t = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * ASM_RUN;
    const int nb = (int)(nseg - e0 < ASM_RUN ? nseg - e0 : ASM_RUN);
    for (int u = t; u <= nb; u += ASM_T) {
        s_ptr[u] = clamp_pos((int64_t)seg_ptr[e0 + u], n_in);
        if (u < nb) s_acc[u] = 0.0;
    }
    __syncthreads();
    const int64_t p1 = s_ptr[nb];
    int64_t pos = s_ptr[0];
    while (pos < p1) {                                                // every quantity that steers this loop is uniform
        int a = 0, b = nb;                                            // the segment that holds pos: last a with s_ptr[a] <= pos
        while (b - a > 1) {
            const int m = (a + b) >> 1;
            if (s_ptr[m] <= pos) a = m; else b = m;
        }
        const int64_t end_a = s_ptr[a + 1];
        if (end_a - s_ptr[a] > ASM_CH) {                              // a long segment: its chunks are summed elsewhere
            pos = end_a > pos ? end_a : pos + 1;
            continue;
        }
        const int64_t wend = pos + ASM_PASS < p1 ? pos + ASM_PASS : p1;
        int64_t idx[ASM_K];
#pragma unroll
        for (int k = 0; k < ASM_K; ++k) {
            const int64_t i = pos + t + k * ASM_T;
            idx[k] = i < wend ? (int64_t)perm[i] : -1;
        }
        double v[ASM_K];
#pragma unroll
        for (int k = 0; k < ASM_K; ++k) v[k] = list_value(idx[k], vals, n_own, ghost, n_ghost);
#pragma unroll
        for (int k = 0; k < ASM_K; ++k) s_val[t + k * ASM_T] = v[k];
        __syncthreads();
        for (int u = a + t; u < nb && s_ptr[u] < wend; u += ASM_T) {
            const int64_t b0 = s_ptr[u], b1 = s_ptr[u + 1];
            if (b1 - b0 > ASM_CH) continue;
            const int64_t lo = b0 > pos ? b0 : pos;
            const int64_t hi = b1 < wend ? b1 : wend;
            if (lo >= hi) continue;
            int j = (int)(lo - pos);
            const int je = (int)(hi - pos);
            double s;
            if (lo == b0) s = s_val[j++]; else s = s_acc[u];
            for (; j < je; ++j) s = s + s_val[j];
            s_acc[u] = s;
        }
        __syncthreads();
        pos = wend;
    }
    for (int u = t; u < nb; u += ASM_T) {                             // the loop's last barrier (or the first) published s_acc
        double s = s_acc[u];
        const int64_t b0 = s_ptr[u], len = s_ptr[u + 1] - b0;
        if (partials && len > ASM_CH) {
            const int64_t nch = (len + ASM_CH - 1) / ASM_CH;
            s = partials[partial_slot(b0, 0)];
            for (int64_t c = 1; c < nch; ++c) s = s + partials[partial_slot(b0, c)];
        }
        out[e0 + u] = s;
    }
}

static int64_t tiles_of(int64_t n_in) { return (n_in + ASM_CH - 1) / ASM_CH; }

template <typename S>
static int segments_impl(const int64_t *skey, int64_t n, S *seg_ptr, int64_t *ukey, int64_t *nnz_host, void *work, void *stream)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "assemble_segments: negative size");
    if (!nnz_host) return set_error(HPCLA_ERR_INVALID, "assemble_segments: null nnz_out_host");
    *nnz_host = 0;
    if (!seg_ptr) return set_error(HPCLA_ERR_INVALID, "assemble_segments: null seg_ptr_out");
    hipStream_t s = as_stream(stream);
    if (n == 0) {
        HPCLA_CHECK_HIP(hipMemsetAsync(seg_ptr, 0, sizeof(S), s));
        return HPCLA_OK;
    }
    if ((uint64_t)n > (uint64_t)(sizeof(S) == 4 ? INT32_MAX : INT64_MAX))
        return set_error(HPCLA_ERR_INVALID, "assemble_segments: n does not fit the position type");
    if (!skey || !ukey || !work) return set_error(HPCLA_ERR_INVALID, "assemble_segments: null array with a non-zero size");
    int64_t *block_sums = static_cast<int64_t *>(work);
    int64_t *total = block_sums + scan_blocks(n);
    if (int rc = exclusive_scan(HeadLoad{skey}, n, HeadEmit<S>{skey, n, seg_ptr, ukey}, block_sums, total, s)) return rc;
    HPCLA_CHECK_HIP(hipMemcpyAsync(nnz_host, total, 8, hipMemcpyDeviceToHost, s));
    HPCLA_CHECK_HIP(hipStreamSynchronize(s));                         // the one synchronisation: the size the caller allocates by
    return HPCLA_OK;
}

template <typename O>
static int row_starts_impl(const int64_t *keys, int64_t n, int64_t nrows, int64_t ncols, int base, O *out, void *stream)
{
    if (n < 0 || nrows < 0 || ncols < 1) return set_error(HPCLA_ERR_INVALID, "assemble_row_starts: need n, nrows >= 0 and ncols >= 1");
    if (base != 0 && base != 1) return set_error(HPCLA_ERR_INVALID, "assemble_row_starts: index_base must be 0 or 1");
    if (nrows > INT64_MAX / ncols) return set_error(HPCLA_ERR_INVALID, "assemble_row_starts: nrows * ncols does not fit 63 bits");
    if ((uint64_t)n + 1 > (uint64_t)(sizeof(O) == 4 ? INT32_MAX : INT64_MAX))
        return set_error(HPCLA_ERR_INVALID, "assemble_row_starts: n does not fit the output type");
    if (!out || (n > 0 && !keys)) return set_error(HPCLA_ERR_INVALID, "assemble_row_starts: null array with a non-zero size");
    const int64_t g = (nrows + 1 + 255) / 256;
    HPCLA_CHECK_GRID(g, "assemble_row_starts");
    assemble_row_starts_kernel<O><<<(uint32_t)g, 256, 0, as_stream(stream)>>>(keys, n, nrows, ncols, base, out);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <typename S>
static int values_impl(const S *seg_ptr, const S *perm, int64_t nseg, int64_t n_in, const double *vals, int64_t n_own,
                       const double *ghost, int64_t n_ghost, int64_t max_len, double *out, void *work, void *stream)
{
    if (nseg < 0 || n_in < 0 || n_own < 0 || n_ghost < 0) return set_error(HPCLA_ERR_INVALID, "assemble_values: negative size");
    if (nseg == 0) return HPCLA_OK;
    if (!seg_ptr || !out || (n_in > 0 && !perm) || (n_own > 0 && !vals) || (n_ghost > 0 && !ghost))
        return set_error(HPCLA_ERR_INVALID, "assemble_values: null array with a non-zero size");
    hipStream_t s = as_stream(stream);
    const bool long_path = n_in > ASM_CH && (max_len < 0 || max_len > ASM_CH);
    if (long_path) {
        if (!work) return set_error(HPCLA_ERR_INVALID, "assemble_values: segments longer than the chunk need the work buffer");
        HPCLA_CHECK_GRID(tiles_of(n_in), "assemble_values");
        assemble_long_kernel<S><<<(uint32_t)tiles_of(n_in), 64, 0, s>>>(seg_ptr, perm, nseg, n_in, vals, n_own, ghost, n_ghost,
                                                                        static_cast<double *>(work));
        HPCLA_CHECK_LAUNCH();
    }
    const int64_t g = (nseg + ASM_RUN - 1) / ASM_RUN;
    HPCLA_CHECK_GRID(g, "assemble_values");
    assemble_values_kernel<S><<<(uint32_t)g, ASM_T, 0, s>>>(seg_ptr, perm, nseg, n_in, vals, n_own, ghost, n_ghost,
                                                           long_path ? static_cast<const double *>(work) : nullptr, out);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_assemble_chunk(void) { return ASM_CH; }
HPCLA_API int64_t hpcla_assemble_run(void) { return ASM_RUN; }
HPCLA_API int64_t hpcla_assemble_pass(void) { return ASM_PASS; }

HPCLA_API int64_t hpcla_assemble_work_bytes(int64_t n)
{
    if (n < 0) return -1;
    return 8 * (scan_blocks(n) + 1) + 64;
}

HPCLA_API int64_t hpcla_assemble_values_work_bytes(int64_t n_in)
{
    if (n_in < 0) return -1;
    return 16 * tiles_of(n_in) + 16;
}

HPCLA_API int hpcla_assemble_keys(const int64_t *rows, const int64_t *cols, int64_t n, int64_t row_lo, int64_t row_hi,
                                  int64_t nrows_global, int64_t ncols, int index_base, int64_t *key_out, int64_t *counts_dev,
                                  void *stream)
{
    if (n < 0 || row_lo < 0 || row_hi < row_lo || nrows_global < row_hi || ncols < 1)
        return set_error(HPCLA_ERR_INVALID, "assemble_keys: need n >= 0, 0 <= row_lo <= row_hi <= nrows_global, ncols >= 1");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "assemble_keys: index_base must be 0 or 1");
    if (row_hi - row_lo > INT64_MAX / ncols)
        return set_error(HPCLA_ERR_INVALID, "assemble_keys: (row_hi - row_lo) * ncols does not fit 63 bits");
    if (!counts_dev) return set_error(HPCLA_ERR_INVALID, "assemble_keys: null counts_dev");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(counts_dev, 0xff, 32, s));         // first positions: -1 (the largest unsigned word) = none
    HPCLA_CHECK_HIP(hipMemsetAsync(counts_dev, 0, 8, s));
    HPCLA_CHECK_HIP(hipMemsetAsync(counts_dev + 2, 0, 8, s));
    if (n == 0) return HPCLA_OK;
    if (!rows || !key_out) return set_error(HPCLA_ERR_INVALID, "assemble_keys: null array with a non-zero size");
    HPCLA_CHECK_GRID((n + 255) / 256, "assemble_keys");
    assemble_keys_kernel<<<(uint32_t)((n + 255) / 256), 256, 0, s>>>(rows, cols, n, row_lo, row_hi, nrows_global, ncols, index_base,
                                                                    key_out, reinterpret_cast<unsigned long long *>(counts_dev));
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_assemble_segments_i32(const int64_t *keys_sorted, int64_t n, int32_t *seg_ptr_out, int64_t *ukey_out,
                                          int64_t *nnz_out_host, void *work, void *stream)
{
    return segments_impl<int32_t>(keys_sorted, n, seg_ptr_out, ukey_out, nnz_out_host, work, stream);
}
HPCLA_API int hpcla_assemble_segments_i64(const int64_t *keys_sorted, int64_t n, int64_t *seg_ptr_out, int64_t *ukey_out,
                                          int64_t *nnz_out_host, void *work, void *stream)
{
    return segments_impl<int64_t>(keys_sorted, n, seg_ptr_out, ukey_out, nnz_out_host, work, stream);
}

HPCLA_API int hpcla_assemble_row_starts_i32(const int64_t *keys_sorted, int64_t n, int64_t nrows, int64_t ncols, int index_base,
                                            int32_t *out, void *stream)
{
    return row_starts_impl<int32_t>(keys_sorted, n, nrows, ncols, index_base, out, stream);
}
HPCLA_API int hpcla_assemble_row_starts_i64(const int64_t *keys_sorted, int64_t n, int64_t nrows, int64_t ncols, int index_base,
                                            int64_t *out, void *stream)
{
    return row_starts_impl<int64_t>(keys_sorted, n, nrows, ncols, index_base, out, stream);
}

HPCLA_API int hpcla_assemble_columns(const int64_t *ukey, int64_t nnz, int64_t ncols, int index_base, int64_t *colidx_out,
                                     void *stream)
{
    if (nnz < 0 || ncols < 1) return set_error(HPCLA_ERR_INVALID, "assemble_columns: need nnz >= 0 and ncols >= 1");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "assemble_columns: index_base must be 0 or 1");
    if (nnz == 0) return HPCLA_OK;
    if (!ukey || !colidx_out) return set_error(HPCLA_ERR_INVALID, "assemble_columns: null array with a non-zero size");
    HPCLA_CHECK_GRID((nnz + 255) / 256, "assemble_columns");
    assemble_columns_kernel<<<(uint32_t)((nnz + 255) / 256), 256, 0, as_stream(stream)>>>(ukey, nnz, ncols, index_base, colidx_out);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_assemble_values_f64_i32(const int32_t *seg_ptr, const int32_t *perm, int64_t nseg, int64_t n_in,
                                            const double *vals, int64_t n_own, const double *ghost, int64_t n_ghost,
                                            int64_t max_len, double *out, void *work, void *stream)
{
    return values_impl<int32_t>(seg_ptr, perm, nseg, n_in, vals, n_own, ghost, n_ghost, max_len, out, work, stream);
}
HPCLA_API int hpcla_assemble_values_f64_i64(const int64_t *seg_ptr, const int64_t *perm, int64_t nseg, int64_t n_in,
                                            const double *vals, int64_t n_own, const double *ghost, int64_t n_ghost,
                                            int64_t max_len, double *out, void *work, void *stream)
{
    return values_impl<int64_t>(seg_ptr, perm, nseg, n_in, vals, n_own, ghost, n_ghost, max_len, out, work, stream);
}
