// amg.hip -- setup kernels and the two fused smoother kernels of the smoothed-aggregation multigrid preconditioner (hp.amg).
// The products of the setup (A T, A P, Pt (A P)), the transpose and the cycle's SpMVs are the library's own; this file holds
// what they do not cover: the level's weights, the strength graph, the aggregation and the prolongator's values.
//
// Rows and columns of A are partitioned alike (n_own == nrows), so a split column c < n_own IS local row c; columns >= n_own
// are ghosts.  Aggregates never cross ranks: the strength graph keeps owned columns only, local row ids as its columns.
//
// weights     per row d = a_ii (0 where none is stored) and sum_j |a_ij| / d over the whole row, ghosts included; a row with
//             !(d > 0) (NaN included) lowers the error word (vector atomic min of the local row).  The row sum is taken by
//             one thread in stored order: s = w ./ d enters P and through it every coarse entry, and a coarse entry that
//             cancels to zero or to rounding noise decides a_ij != 0 one level down, so the sum's order is part of the
//             method's definition (the products have theirs: spgemm.hip) and must not depend on a lane count.
// strength    entry (i, c) kept when c != i, c < n_own, a_ic != 0 and |a_ic| >= theta * sqrt(a_ii * a_cc): count through the
//             shared scan (scan.h), then fill, one thread per row, entries in the row's own order.
// roots       distance-2 maximal independent set (Bell, Dalton, Olson).  key_i = (h(global row) << 31) | local row, all
//             distinct and < 2^62.  state k_i: the key (undecided), 2^62 (root) or -1 (out).  A round is three launches on
//             double-buffered arrays: m1 = max(k, neighbours' k), m2 = max(m1, neighbours' m1), decide (undecided and
//             m2 == key: root; undecided and m2 >= 2^62: out) with the workgroup's count of rows still undecided.  The host
//             sums the counts and stops at zero.  No atomics, no kernel waits for another.
// join        pass 1: a root owns itself, a non-root takes the neighbouring root with the largest key (its local row is the
//             key's low 31 bits); pass 2: a row still free takes the owner of the owned neighbour with the largest key.
//             Every row is within distance 2 of a root, so none stays free; one that did would lower the error word.
//             Roots are numbered by the scan of the root flags in row order.
// P           p_ic = [c == agg(i)] - s_i * (A T)_ic on the stored pattern of A T (global columns through col_indices).
//
// For a nonsymmetric A (hp.amg(A, symmetric=False)) two more entries:
// symmetrise  the roots and the join assume an undirected graph, so the strength graph E becomes E u E^T on the device:
//             hpcla_amg_symmetrise_count adds the in-degrees of E (one integer atomic per edge) to its out-degrees and scans
//             them (scan.h) into the combined row pointer; hpcla_amg_symmetrise_fill copies each row's out-list, sets the
//             row's cursor behind it, and every edge (i, c) then takes a slot of row c through an integer atomic on c's cursor
//             and stores i there.  Every store is bounded by the row's end.  The order of a row's in-list follows the order
//             the atomics happen to be served in, and an edge stored in both directions appears twice; the neighbour maxima
//             and the join take maxima over distinct keys, which depend on the SET of a row's neighbours only, so two builds
//             give identical aggregates all the same.  Ghost columns are in neither E nor E^T.  The graph has one index form
//             (int64 row pointer, int32 local columns) whatever A's is.  No float atomics, no kernel waits for another.
// R           r_cj = [agg(j) == c] - (T^t A)_cj * s_j on the stored pattern of T^t A: the Petrov-Galerkin restriction
//             T^t (I - A S).  Its columns are the level's rows, all owned (one rank).
//
// With near-nullspace candidates (hp.amg(A, B=...), k <= 8 = AMG_G columns) three more entries:
// fit         per aggregate B[members, :] = Q R by classical Gram-Schmidt run twice, the members ascending: Q goes to the rows
//             of the dense n x k array Tv (row i: the k values of row i of T), R to rows k a .. k a + k - 1 of the next level's
//             candidates, +0.0 below the diagonal.  The arithmetic is part of the method's definition.  Column j, v = B[members, j]:
//             n0 = sqrt(sum v_m^2); twice: h_c = sum_m q_c[m] v[m] for every c < j, all taken before any update, then
//             v[m] = v[m] - h_c q_c[m] for c ascending; R_cj = the first pass's h_c plus the second's; nr = sqrt(sum v_m^2),
//             R_jj = nr, q_j = v / nr (a division).  Every sum over the members belongs to ONE lane, which adds in ascending
//             member order from +0.0.  !(nr > 1e-10 n0) (a zero column and NaN included) drops the column: q_j = 0, row j of R
//             = 0, the column takes no part in later ones, and the error word is lowered to 8 a + j (vector atomic min), so the
//             smallest aggregate's first dropped column is what the host reads.  One group per aggregate: lanes c < j take the
//             dot products of a pass side by side, lane j the norms, the updates stride the members over the group; v lives in
//             its final place in Tv.  An aggregate of any size loops.  No LDS, no float atomics.
// P, R with B the two value kernels with T's k entries per row: p_e = (col / k == agg(i) ? Tv[i, col - k agg(i)] : 0) - s_i at_e,
//             r_cj = (agg(j) == c / k ? Tv[j, c - k agg(j)] : 0) - ta_cj s_j.
//
// A group of AMG_G = 8 lanes serves one row in the neighbour loops (8 rows per wave): the grids and their coarse levels
// store 5 to about 30 entries per row, so a whole wave per row would idle most lanes; a longer row loops in steps of 8.
// Products and sums are separately rounded (-ffp-contract=off).  No instantiation uses scratch.
#include "common.h"
#include "scan.h"

namespace hpcla {

constexpr int AMG_THREADS = 256;
constexpr int AMG_G = 8;
constexpr int64_t AMG_ROOT = (int64_t)1 << 62;
constexpr int64_t AMG_MASK31 = ((int64_t)1 << 31) - 1;

__device__ __forceinline__ int64_t amg_group_max(int64_t v)
{
#pragma unroll
    for (int off = AMG_G / 2; off > 0; off >>= 1) {
        const int64_t t = __shfl_xor(v, off, AMG_G);
        v = t > v ? t : v;
    }
    return v;
}

static inline uint32_t amg_group_grid(int64_t nrows) { return (uint32_t)((nrows * AMG_G + AMG_THREADS - 1) / AMG_THREADS); }
static inline uint32_t amg_row_grid(int64_t nrows) { return (uint32_t)((nrows + AMG_THREADS - 1) / AMG_THREADS); }

template <typename I>
__global__ __launch_bounds__(AMG_THREADS) void amg_weights_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                  const double *__restrict__ nzval, int64_t nrows, int base,
                                                                  double *__restrict__ diag, double *__restrict__ ratio,
                                                                  int64_t *__restrict__ info)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int64_t e0 = (int64_t)rowptr[i] - base, e1 = (int64_t)rowptr[i + 1] - base;
    double sum = 0.0, d = 0.0;
    for (int64_t e = e0; e < e1; ++e) {                      // one thread, stored order: see the note on the weights above
        const double v = nzval[e];
        sum = sum + fabs(v);
        if ((int64_t)colval[e] - base == i) d = v;
    }
    diag[i] = d;
    ratio[i] = sum / d;
    if (!(d > 0.0)) atomicMin(reinterpret_cast<unsigned long long *>(info), (unsigned long long)i);
}

__global__ __launch_bounds__(AMG_THREADS) void amg_smoother_kernel(double w, const double *__restrict__ diag,
                                                                   double *__restrict__ s, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i < n) s[i] = w / diag[i];
}

__device__ __forceinline__ bool amg_strong(int64_t i, int64_t c, double v, const double *__restrict__ diag, int64_t n_own,
                                           double theta)
{
    if (c == i || c >= n_own || c < 0 || v == 0.0) return false;
    return fabs(v) >= theta * sqrt(diag[i] * diag[c]);
}

template <typename I>
struct AmgStrengthLoad {
    const I *rowptr, *colval;
    const double *nzval, *diag;
    int base;
    int64_t n_own;
    double theta;
    __device__ int64_t operator()(int64_t i) const
    {
        const int64_t e0 = (int64_t)rowptr[i] - base, e1 = (int64_t)rowptr[i + 1] - base;
        int64_t m = 0;
        for (int64_t e = e0; e < e1; ++e) m += amg_strong(i, (int64_t)colval[e] - base, nzval[e], diag, n_own, theta) ? 1 : 0;
        return m;
    }
};

struct AmgRowptrEmit {
    int64_t nrows;
    int64_t *s_rowptr, *total;
    __device__ void operator()(int64_t i, int64_t before, int64_t m) const
    {
        s_rowptr[i] = before;
        if (i == nrows - 1) {
            s_rowptr[nrows] = before + m;
            total[0] = before + m;
        }
    }
};

template <typename I>
__global__ __launch_bounds__(AMG_THREADS) void amg_strength_fill_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                        const double *__restrict__ nzval,
                                                                        const double *__restrict__ diag, int64_t nrows, int base,
                                                                        int64_t n_own, double theta,
                                                                        const int64_t *__restrict__ s_rowptr,
                                                                        int32_t *__restrict__ s_cols)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int64_t e0 = (int64_t)rowptr[i] - base, e1 = (int64_t)rowptr[i + 1] - base;
    int64_t pos = s_rowptr[i];
    const int64_t end = s_rowptr[i + 1];
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t c = (int64_t)colval[e] - base;
        if (amg_strong(i, c, nzval[e], diag, n_own, theta) && pos < end) s_cols[pos++] = (int32_t)c;
    }
}

// indeg[c] += 1 for every edge (i, c) of the graph; a group of lanes per row
__global__ __launch_bounds__(AMG_THREADS) void amg_indegree_kernel(const int64_t *__restrict__ s_rowptr,
                                                                   const int32_t *__restrict__ s_cols, int64_t nrows,
                                                                   int64_t *__restrict__ indeg)
{
    const int64_t i = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (i >= nrows) return;
    for (int64_t e = s_rowptr[i] + l; e < s_rowptr[i + 1]; e += AMG_G) {
        const int64_t c = s_cols[e];
        if (c >= 0 && c < nrows) atomicAdd(reinterpret_cast<unsigned long long *>(indeg + c), 1ULL);
    }
}

struct AmgDegreeLoad {
    const int64_t *s_rowptr, *indeg;
    __device__ int64_t operator()(int64_t i) const { return s_rowptr[i + 1] - s_rowptr[i] + indeg[i]; }
};

// row i of the combined graph starts with its out-list; cursor[i] is left behind it
__global__ __launch_bounds__(AMG_THREADS) void amg_symmetrise_copy_kernel(const int64_t *__restrict__ s_rowptr,
                                                                          const int32_t *__restrict__ s_cols, int64_t nrows,
                                                                          const int64_t *__restrict__ u_rowptr,
                                                                          int64_t *__restrict__ cursor, int32_t *__restrict__ u_cols)
{
    const int64_t i = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (i >= nrows) return;
    const int64_t e0 = s_rowptr[i], m = s_rowptr[i + 1] - e0;
    const int64_t pos = u_rowptr[i], end = u_rowptr[i + 1];
    for (int64_t k = l; k < m; k += AMG_G)
        if (pos + k < end) u_cols[pos + k] = s_cols[e0 + k];
    if (l == 0) cursor[i] = pos + m < end ? pos + m : end;
}

// edge (i, c): row c takes i into the next free slot of its in-list
__global__ __launch_bounds__(AMG_THREADS) void amg_symmetrise_scatter_kernel(const int64_t *__restrict__ s_rowptr,
                                                                             const int32_t *__restrict__ s_cols, int64_t nrows,
                                                                             const int64_t *__restrict__ u_rowptr,
                                                                             int64_t *__restrict__ cursor,
                                                                             int32_t *__restrict__ u_cols)
{
    const int64_t i = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (i >= nrows) return;
    for (int64_t e = s_rowptr[i] + l; e < s_rowptr[i + 1]; e += AMG_G) {
        const int64_t c = s_cols[e];
        if (c < 0 || c >= nrows) continue;
        const int64_t pos = (int64_t)atomicAdd(reinterpret_cast<unsigned long long *>(cursor + c), 1ULL);
        if (pos >= u_rowptr[c] && pos < u_rowptr[c + 1]) u_cols[pos] = (int32_t)i;
    }
}

__device__ __forceinline__ int64_t amg_hash31(int64_t g)
{
    uint64_t x = (uint64_t)(g + 1) * 0x9E3779B97F4A7C15ULL;
    x ^= x >> 32;
    x *= 0xD6E8FEB86659FD93ULL;
    x ^= x >> 32;
    return (int64_t)(x >> 33);
}

__global__ __launch_bounds__(AMG_THREADS) void amg_mis_init_kernel(int64_t nrows, int64_t row_start, int64_t *__restrict__ key,
                                                                   int64_t *__restrict__ state)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int64_t k = (amg_hash31(row_start + i) << 31) | i;
    key[i] = k;
    state[i] = k;
}

// out_i = max(in_i, max over the strong neighbours j of in_j)
__global__ __launch_bounds__(AMG_THREADS) void amg_neighbour_max_kernel(const int64_t *__restrict__ s_rowptr,
                                                                        const int32_t *__restrict__ s_cols, int64_t nrows,
                                                                        const int64_t *__restrict__ in, int64_t *__restrict__ out)
{
    const int64_t i = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (i >= nrows) return;
    int64_t m = in[i];
    for (int64_t e = s_rowptr[i] + l; e < s_rowptr[i + 1]; e += AMG_G) {
        const int64_t t = in[s_cols[e]];
        m = t > m ? t : m;
    }
    m = amg_group_max(m);
    if (l == 0) out[i] = m;
}

__global__ __launch_bounds__(AMG_THREADS) void amg_mis_decide_kernel(const int64_t *__restrict__ key, const int64_t *__restrict__ m2,
                                                                     const int64_t *__restrict__ state_in,
                                                                     int64_t *__restrict__ state_out, int64_t nrows,
                                                                     int64_t *__restrict__ block_undecided)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    int undecided = 0;
    if (i < nrows) {
        int64_t k = state_in[i];
        if (k >= 0 && k < AMG_ROOT) {
            const int64_t m = m2[i];
            if (m == key[i]) k = AMG_ROOT;
            else if (m >= AMG_ROOT) k = -1;
            else undecided = 1;
        }
        state_out[i] = k;
    }
    const int total = __syncthreads_count(undecided);
    if (threadIdx.x == 0) block_undecided[blockIdx.x] = total;
}

// PASS 1: owner = the row itself (root), the neighbouring root with the largest key, or -1
// PASS 2: owner = prev's, or the owner of the owned neighbour with the largest key; -1 lowers the error word
template <int PASS>
__global__ __launch_bounds__(AMG_THREADS) void amg_join_kernel(const int64_t *__restrict__ s_rowptr, const int32_t *__restrict__ s_cols,
                                                               int64_t nrows, const int64_t *__restrict__ key,
                                                               const int64_t *__restrict__ state, const int32_t *__restrict__ prev,
                                                               int32_t *__restrict__ owner, int64_t *__restrict__ info)
{
    const int64_t i = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (i >= nrows) return;
    int32_t o = PASS == 1 ? (state[i] == AMG_ROOT ? (int32_t)i : -1) : prev[i];
    if (o < 0) {                                             // the same in every lane of the group
        int64_t best = -1;
        for (int64_t e = s_rowptr[i] + l; e < s_rowptr[i + 1]; e += AMG_G) {
            const int32_t j = s_cols[e];
            const bool ok = PASS == 1 ? state[j] == AMG_ROOT : prev[j] >= 0;
            const int64_t t = ok ? key[j] : -1;
            best = t > best ? t : best;
        }
        best = amg_group_max(best);
        if (best >= 0) o = PASS == 1 ? (int32_t)(best & AMG_MASK31) : prev[best & AMG_MASK31];
    }
    if (l == 0) {
        owner[i] = o;
        if (PASS == 2 && o < 0) atomicMin(reinterpret_cast<unsigned long long *>(info), (unsigned long long)i);
    }
}

struct AmgRootLoad {
    const int64_t *state;
    __device__ int64_t operator()(int64_t i) const { return state[i] == AMG_ROOT ? 1 : 0; }
};

struct AmgRootEmit {
    int64_t nrows;
    int64_t *rootid, *total;
    __device__ void operator()(int64_t i, int64_t before, int64_t v) const
    {
        rootid[i] = before;
        if (i == nrows - 1) total[0] = before + v;
    }
};

__global__ __launch_bounds__(AMG_THREADS) void amg_ids_kernel(const int32_t *__restrict__ owner, const int64_t *__restrict__ rootid,
                                                              int64_t nrows, int64_t offset, int64_t *__restrict__ agg)
{
    const int64_t i = (int64_t)blockIdx.x * AMG_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int32_t o = owner[i];
    agg[i] = offset + (o >= 0 && o < nrows ? rootid[o] : 0);
}

template <typename I>
__global__ __launch_bounds__(AMG_THREADS) void amg_prolongator_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                      const int64_t *__restrict__ col_indices,
                                                                      const double *__restrict__ at, const int64_t *__restrict__ agg,
                                                                      const double *__restrict__ s, int64_t nrows, int base,
                                                                      double *__restrict__ p)
{
    const int64_t i = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (i >= nrows) return;
    const int64_t mine = agg[i];
    const double si = s[i];
    const int64_t e0 = (int64_t)rowptr[i] - base, e1 = (int64_t)rowptr[i + 1] - base;
    for (int64_t e = e0 + l; e < e1; e += AMG_G) {
        const double one = col_indices[(int64_t)colval[e] - base] == mine ? 1.0 : 0.0;
        p[e] = one - si * at[e];
    }
}

// row c of T^t A (the aggregate row_offset + c): r_cj = [agg(j) == row_offset + c] - ta_cj * s_j; a column outside 0..ncols is left
template <typename I>
__global__ __launch_bounds__(AMG_THREADS) void amg_restrictor_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                     const int64_t *__restrict__ col_indices,
                                                                     const double *__restrict__ ta, const int64_t *__restrict__ agg,
                                                                     const double *__restrict__ s, int64_t nrows, int64_t ncols,
                                                                     int64_t row_offset, int base, double *__restrict__ r)
{
    const int64_t c = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (c >= nrows) return;
    const int64_t mine = row_offset + c;
    const int64_t e0 = (int64_t)rowptr[c] - base, e1 = (int64_t)rowptr[c + 1] - base;
    for (int64_t e = e0 + l; e < e1; e += AMG_G) {
        const int64_t j = col_indices[(int64_t)colval[e] - base];
        if (j < 0 || j >= ncols) continue;
        const double one = agg[j] == mine ? 1.0 : 0.0;
        r[e] = one - ta[e] * s[j];
    }
}

__device__ __forceinline__ double amg_group_get(double v, int lane) { return __shfl(v, lane, AMG_G); }

// What one lane has written to Tv, the other lanes of its group read: the group is part of one wave, whose loads and stores go
// through one vector cache in the order they were issued, so a workgroup-scope fence is all it takes: it keeps the compiler from
// moving an access across it and costs no cache operation.
__device__ __forceinline__ void amg_group_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

// B[members of aggregate a, :] = Q R, K columns, the group's lane l = threadIdx & 7.  Column j, see the note on the fit above:
//   pass 1    lane c < j: h_c = sum_m q_c[m] * b[m]; lane j: sum_m b[m]^2 (n0).  Sequential, ascending member order, from +0.0.
//   update 1  v[m] = b[m] - h_0 q_0[m] - ... - h_{j-1} q_{j-1}[m] into Tv, the members strided over the group.
//   pass 2    lane c < j: h'_c = sum_m q_c[m] * v[m];  update 2 in place (a lane updates the members it wrote);  R_cj = h_c + h'_c.
//   norm      lane j: nr = sqrt(sum_m v[m]^2);  q_j = v / nr, R_jj = nr;  or the drop.
// A member outside 0..nrows is passed over (no load, no store).  No shuffle stands inside a loop whose trip count differs
// between the lanes of a group.
template <int K>
__global__ __launch_bounds__(AMG_THREADS) void amg_fit_kernel(const double *__restrict__ b, int64_t nrows,
                                                              const int64_t *__restrict__ mptr, const int64_t *__restrict__ members,
                                                              int64_t n_members, int64_t n_agg, double *tv, double *__restrict__ bc,
                                                              int64_t *__restrict__ info)
{
    const int64_t a = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (a >= n_agg) return;
    int64_t e0 = mptr[a], e1 = mptr[a + 1];
    e0 = e0 < 0 ? 0 : (e0 > n_members ? n_members : e0);
    e1 = e1 < e0 ? e0 : (e1 > n_members ? n_members : e1);
    const int64_t m = e1 - e0;
    constexpr int H = K > 1 ? K - 1 : 1;
    bool dropped = false;                                    // of column l
    for (int j = 0; j < K; ++j) {
        double h1 = 0.0;
        if (l <= j) {
            for (int64_t t = 0; t < m; ++t) {
                const int64_t r = members[e0 + t];
                if (r < 0 || r >= nrows) continue;
                const double v = b[r * K + j];
                const double x = l < j ? tv[r * K + l] : v;
                h1 = h1 + x * v;
            }
        }
        if (l < j && dropped) h1 = 0.0;
        const double n0 = sqrt(amg_group_get(h1, j));
        double hc[H];
#pragma unroll
        for (int c = 0; c < H; ++c) hc[c] = amg_group_get(h1, c);
        for (int64_t t = l; t < m; t += AMG_G) {
            const int64_t r = members[e0 + t];
            if (r < 0 || r >= nrows) continue;
            double v = b[r * K + j];
#pragma unroll
            for (int c = 0; c < H; ++c)
                if (c < j) v = v - hc[c] * tv[r * K + c];
            tv[r * K + j] = v;
        }
        amg_group_fence();
        double h2 = 0.0;
        if (l < j && !dropped) {
            for (int64_t t = 0; t < m; ++t) {
                const int64_t r = members[e0 + t];
                if (r < 0 || r >= nrows) continue;
                h2 = h2 + tv[r * K + l] * tv[r * K + j];
            }
        }
#pragma unroll
        for (int c = 0; c < H; ++c) hc[c] = amg_group_get(h2, c);
        for (int64_t t = l; t < m; t += AMG_G) {
            const int64_t r = members[e0 + t];
            if (r < 0 || r >= nrows) continue;
            double v = tv[r * K + j];
#pragma unroll
            for (int c = 0; c < H; ++c)
                if (c < j) v = v - hc[c] * tv[r * K + c];
            tv[r * K + j] = v;
        }
        amg_group_fence();
        double sq = 0.0;
        if (l == j) {
            for (int64_t t = 0; t < m; ++t) {
                const int64_t r = members[e0 + t];
                if (r < 0 || r >= nrows) continue;
                const double v = tv[r * K + j];
                sq = sq + v * v;
            }
        }
        const double nr = sqrt(amg_group_get(sq, j));
        const bool drop = !(nr > 1e-10 * n0);
        for (int64_t t = l; t < m; t += AMG_G) {
            const int64_t r = members[e0 + t];
            if (r < 0 || r >= nrows) continue;
            tv[r * K + j] = drop ? 0.0 : tv[r * K + j] / nr;
        }
        amg_group_fence();
        if (l < K) {
            double rv = 0.0;                                 // below the diagonal, and the row of a dropped column
            if (l < j) rv = h1 + h2;
            else if (l == j && !drop) rv = nr;
            bc[(a * K + l) * K + j] = rv;
        }
        if (l == j && drop) {
            dropped = true;
            atomicMin(reinterpret_cast<unsigned long long *>(info), (unsigned long long)(a * AMG_G + j));
        }
    }
}

// as amg_prolongator_kernel with K columns per aggregate: the global column c belongs to aggregate c / K
template <typename I>
__global__ __launch_bounds__(AMG_THREADS) void amg_prolongator_b_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                        const int64_t *__restrict__ col_indices,
                                                                        const double *__restrict__ at, const int64_t *__restrict__ agg,
                                                                        const double *__restrict__ s, const double *__restrict__ tv,
                                                                        int64_t k, int64_t nrows, int base, double *__restrict__ p)
{
    const int64_t i = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (i >= nrows) return;
    const int64_t first = agg[i] * k;                        // the columns first .. first + k - 1 are the row's own
    const double si = s[i];
    const int64_t e0 = (int64_t)rowptr[i] - base, e1 = (int64_t)rowptr[i + 1] - base;
    for (int64_t e = e0 + l; e < e1; e += AMG_G) {
        const int64_t c = col_indices[(int64_t)colval[e] - base] - first;
        const double t = c >= 0 && c < k ? tv[i * k + c] : 0.0;
        p[e] = t - si * at[e];
    }
}

// as amg_restrictor_kernel: row c of T^t A is the coarse unknown row_offset + c of the aggregate (row_offset + c) / K
template <typename I>
__global__ __launch_bounds__(AMG_THREADS) void amg_restrictor_b_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                       const int64_t *__restrict__ col_indices,
                                                                       const double *__restrict__ ta, const int64_t *__restrict__ agg,
                                                                       const double *__restrict__ s, const double *__restrict__ tv,
                                                                       int64_t k, int64_t nrows, int64_t ncols, int64_t row_offset,
                                                                       int base, double *__restrict__ r)
{
    const int64_t c = ((int64_t)blockIdx.x * AMG_THREADS + threadIdx.x) / AMG_G;
    const int l = threadIdx.x & (AMG_G - 1);
    if (c >= nrows) return;
    const int64_t mine = (row_offset + c) / k, part = (row_offset + c) % k;
    const int64_t e0 = (int64_t)rowptr[c] - base, e1 = (int64_t)rowptr[c + 1] - base;
    for (int64_t e = e0 + l; e < e1; e += AMG_G) {
        const int64_t j = col_indices[(int64_t)colval[e] - base];
        if (j < 0 || j >= ncols) continue;
        const double t = agg[j] == mine ? tv[j * k + part] : 0.0;
        r[e] = t - ta[e] * s[j];
    }
}

// MODE 0: x = s .* b          MODE 1: x = x + s .* (b - t)         (16-byte accesses, the odd element by one thread)
template <int MODE>
__global__ __launch_bounds__(256) void amg_smooth_kernel(const double *__restrict__ s, const double *__restrict__ b,
                                                         const double *__restrict__ t, double *__restrict__ x, int64_t n)
{
    const int64_t n2 = n / 2;
    const double2 *s2 = reinterpret_cast<const double2 *>(s), *b2 = reinterpret_cast<const double2 *>(b);
    const double2 *t2 = reinterpret_cast<const double2 *>(t);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n2; i += stride) {
        const double2 sv = s2[i], bv = b2[i];
        double2 xv;
        if (MODE == 0) {
            xv.x = sv.x * bv.x;
            xv.y = sv.y * bv.y;
        } else {
            const double2 tv = t2[i];
            xv = x2[i];
            xv.x = xv.x + sv.x * (bv.x - tv.x);
            xv.y = xv.y + sv.y * (bv.y - tv.y);
        }
        x2[i] = xv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        if (MODE == 0) x[j] = s[j] * b[j];
        else x[j] = x[j] + s[j] * (b[j] - t[j]);
    }
}

static int amg_check_rows(const char *what, int64_t nrows, int64_t n_own, int index_base)
{
    if (nrows < 0 || n_own != nrows) return set_error(HPCLA_ERR_INVALID, "%s: needs n_own == nrows >= 0", what);
    if (nrows > 0x7fffffffLL) return set_error(HPCLA_ERR_UNSUPPORTED, "%s: at most 2^31 - 1 rows per rank", what);
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "%s: index_base must be 0 or 1", what);
    return HPCLA_OK;
}

template <typename I>
static int amg_weights_impl(const I *rowptr, const I *colval, const double *nzval, int64_t nrows, int64_t n_own, int index_base,
                            double *diag, double *ratio, int64_t *info, void *stream)
{
    int rc = amg_check_rows("amg_weights", nrows, n_own, index_base);
    if (rc) return rc;
    if (!info) return set_error(HPCLA_ERR_INVALID, "amg_weights: null info");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(info, 0xff, sizeof(int64_t), s));
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr || !colval || !nzval || !diag || !ratio) return set_error(HPCLA_ERR_INVALID, "amg_weights: null array");
    amg_weights_kernel<I><<<amg_row_grid(nrows), AMG_THREADS, 0, s>>>(rowptr, colval, nzval, nrows, index_base, diag, ratio, info);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <typename I>
static int amg_strength_count_impl(const I *rowptr, const I *colval, const double *nzval, const double *diag, int64_t nrows,
                                   int64_t n_own, int index_base, double theta, int64_t *s_rowptr, int64_t *info, void *work,
                                   void *stream)
{
    int rc = amg_check_rows("amg_strength_count", nrows, n_own, index_base);
    if (rc) return rc;
    if (!(theta >= 0.0 && theta < 1.0)) return set_error(HPCLA_ERR_INVALID, "amg_strength_count: theta must lie in [0, 1)");
    if (!s_rowptr || !info || !work) return set_error(HPCLA_ERR_INVALID, "amg_strength_count: null rowptr / info / work");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(info, 0, sizeof(int64_t), s));
    if (nrows == 0) {
        HPCLA_CHECK_HIP(hipMemsetAsync(s_rowptr, 0, sizeof(int64_t), s));
        return HPCLA_OK;
    }
    if (!rowptr || !colval || !nzval || !diag) return set_error(HPCLA_ERR_INVALID, "amg_strength_count: null array");
    int64_t *sums = reinterpret_cast<int64_t *>(work);
    return exclusive_scan(AmgStrengthLoad<I>{rowptr, colval, nzval, diag, index_base, n_own, theta}, nrows,
                          AmgRowptrEmit{nrows, s_rowptr, info}, sums + 1, sums, s);
}

template <typename I>
static int amg_strength_fill_impl(const I *rowptr, const I *colval, const double *nzval, const double *diag, int64_t nrows,
                                  int64_t n_own, int index_base, double theta, const int64_t *s_rowptr, int32_t *s_cols,
                                  void *stream)
{
    int rc = amg_check_rows("amg_strength_fill", nrows, n_own, index_base);
    if (rc) return rc;
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr || !colval || !nzval || !diag || !s_rowptr || !s_cols)
        return set_error(HPCLA_ERR_INVALID, "amg_strength_fill: null array");
    amg_strength_fill_kernel<I><<<amg_row_grid(nrows), AMG_THREADS, 0, as_stream(stream)>>>(rowptr, colval, nzval, diag, nrows,
                                                                                           index_base, n_own, theta, s_rowptr,
                                                                                           s_cols);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <typename I>
static int amg_prolongator_impl(const I *rowptr, const I *colval, const int64_t *col_indices, const double *at,
                                const int64_t *agg, const double *s_dev, int64_t nrows, int index_base, double *p, void *stream)
{
    if (nrows < 0) return set_error(HPCLA_ERR_INVALID, "amg_prolongator: negative size");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "amg_prolongator: index_base must be 0 or 1");
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr || !colval || !col_indices || !at || !agg || !s_dev || !p)
        return set_error(HPCLA_ERR_INVALID, "amg_prolongator: null array");
    HPCLA_CHECK_GRID((nrows * AMG_G + AMG_THREADS - 1) / AMG_THREADS, "amg_prolongator");
    amg_prolongator_kernel<I><<<amg_group_grid(nrows), AMG_THREADS, 0, as_stream(stream)>>>(rowptr, colval, col_indices, at, agg,
                                                                                           s_dev, nrows, index_base, p);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <typename I>
static int amg_restrictor_impl(const I *rowptr, const I *colval, const int64_t *col_indices, const double *ta, const int64_t *agg,
                               const double *s_dev, int64_t nrows, int64_t ncols, int64_t row_offset, int index_base, double *r,
                               void *stream)
{
    if (nrows < 0 || ncols < 0 || row_offset < 0) return set_error(HPCLA_ERR_INVALID, "amg_restrictor: negative size or offset");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "amg_restrictor: index_base must be 0 or 1");
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr || !colval || !col_indices || !ta || !agg || !s_dev || !r)
        return set_error(HPCLA_ERR_INVALID, "amg_restrictor: null array");
    HPCLA_CHECK_GRID((nrows * AMG_G + AMG_THREADS - 1) / AMG_THREADS, "amg_restrictor");
    amg_restrictor_kernel<I><<<amg_group_grid(nrows), AMG_THREADS, 0, as_stream(stream)>>>(rowptr, colval, col_indices, ta, agg,
                                                                                          s_dev, nrows, ncols, row_offset,
                                                                                          index_base, r);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <int K>
static void amg_fit_launch(const double *b, int64_t nrows, const int64_t *mptr, const int64_t *members, int64_t n_members,
                           int64_t n_agg, double *tv, double *bc, int64_t *info, hipStream_t s)
{
    amg_fit_kernel<K><<<amg_group_grid(n_agg), AMG_THREADS, 0, s>>>(b, nrows, mptr, members, n_members, n_agg, tv, bc, info);
}

template <typename I>
static int amg_prolongator_b_impl(const I *rowptr, const I *colval, const int64_t *col_indices, const double *at,
                                  const int64_t *agg, const double *s_dev, const double *tv, int k, int64_t nrows, int index_base,
                                  double *p, void *stream)
{
    if (nrows < 0) return set_error(HPCLA_ERR_INVALID, "amg_prolongator_b: negative size");
    if (k < 1 || k > AMG_G) return set_error(HPCLA_ERR_INVALID, "amg_prolongator_b: k must lie in 1..8");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "amg_prolongator_b: index_base must be 0 or 1");
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr || !colval || !col_indices || !at || !agg || !s_dev || !tv || !p)
        return set_error(HPCLA_ERR_INVALID, "amg_prolongator_b: null array");
    HPCLA_CHECK_GRID((nrows * AMG_G + AMG_THREADS - 1) / AMG_THREADS, "amg_prolongator_b");
    amg_prolongator_b_kernel<I><<<amg_group_grid(nrows), AMG_THREADS, 0, as_stream(stream)>>>(rowptr, colval, col_indices, at, agg,
                                                                                             s_dev, tv, k, nrows, index_base, p);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <typename I>
static int amg_restrictor_b_impl(const I *rowptr, const I *colval, const int64_t *col_indices, const double *ta, const int64_t *agg,
                                 const double *s_dev, const double *tv, int k, int64_t nrows, int64_t ncols, int64_t row_offset,
                                 int index_base, double *r, void *stream)
{
    if (nrows < 0 || ncols < 0 || row_offset < 0) return set_error(HPCLA_ERR_INVALID, "amg_restrictor_b: negative size or offset");
    if (k < 1 || k > AMG_G) return set_error(HPCLA_ERR_INVALID, "amg_restrictor_b: k must lie in 1..8");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "amg_restrictor_b: index_base must be 0 or 1");
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr || !colval || !col_indices || !ta || !agg || !s_dev || !tv || !r)
        return set_error(HPCLA_ERR_INVALID, "amg_restrictor_b: null array");
    HPCLA_CHECK_GRID((nrows * AMG_G + AMG_THREADS - 1) / AMG_THREADS, "amg_restrictor_b");
    amg_restrictor_b_kernel<I><<<amg_group_grid(nrows), AMG_THREADS, 0, as_stream(stream)>>>(rowptr, colval, col_indices, ta, agg,
                                                                                            s_dev, tv, k, nrows, ncols, row_offset,
                                                                                            index_base, r);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <int MODE>
static int amg_smooth_impl(const double *s_dev, const double *b, const double *t, double *x, int64_t n, void *stream)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "amg_smooth: negative size");
    if (n == 0) return HPCLA_OK;
    if (!s_dev || !b || !x || (MODE == 1 && !t)) return set_error(HPCLA_ERR_INVALID, "amg_smooth: null pointer");
    if ((reinterpret_cast<uintptr_t>(s_dev) & 15) || (reinterpret_cast<uintptr_t>(b) & 15) || (reinterpret_cast<uintptr_t>(x) & 15) ||
        (MODE == 1 && (reinterpret_cast<uintptr_t>(t) & 15)))
        return set_error(HPCLA_ERR_INVALID, "amg_smooth: vectors must be 16-byte aligned");
    int64_t g = (n / 2 + 255) / 256;
    g = g < 1 ? 1 : (g > 4096 ? 4096 : g);
    amg_smooth_kernel<MODE><<<(uint32_t)g, 256, 0, as_stream(stream)>>>(s_dev, b, t, x, n);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_amg_work_bytes(int64_t nrows)
{
    if (nrows < 0) return -1;
    return (int64_t)sizeof(int64_t) * (1 + scan_blocks(nrows > 0 ? nrows : 1));
}

HPCLA_API int64_t hpcla_amg_round_blocks(int64_t nrows)
{
    if (nrows < 0) return -1;
    return nrows > 0 ? (nrows + AMG_THREADS - 1) / AMG_THREADS : 1;
}

HPCLA_API int hpcla_amg_weights_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval, int64_t nrows,
                                        int64_t n_own, int index_base, double *diag_dev, double *ratio_dev, int64_t *info_dev,
                                        void *stream)
{
    return amg_weights_impl<int32_t>(rowptr, colval_split, nzval, nrows, n_own, index_base, diag_dev, ratio_dev, info_dev, stream);
}

HPCLA_API int hpcla_amg_weights_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval, int64_t nrows,
                                        int64_t n_own, int index_base, double *diag_dev, double *ratio_dev, int64_t *info_dev,
                                        void *stream)
{
    return amg_weights_impl<int64_t>(rowptr, colval_split, nzval, nrows, n_own, index_base, diag_dev, ratio_dev, info_dev, stream);
}

HPCLA_API int hpcla_amg_smoother_f64(double w, const double *diag_dev, double *s_dev, int64_t n, void *stream)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "amg_smoother: negative size");
    if (n == 0) return HPCLA_OK;
    if (!diag_dev || !s_dev) return set_error(HPCLA_ERR_INVALID, "amg_smoother: null pointer");
    HPCLA_CHECK_GRID((n + AMG_THREADS - 1) / AMG_THREADS, "amg_smoother");
    amg_smoother_kernel<<<amg_row_grid(n), AMG_THREADS, 0, as_stream(stream)>>>(w, diag_dev, s_dev, n);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_amg_strength_count_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                               const double *diag_dev, int64_t nrows, int64_t n_own, int index_base, double theta,
                                               int64_t *s_rowptr_dev, int64_t *info_dev, void *work, void *stream)
{
    return amg_strength_count_impl<int32_t>(rowptr, colval_split, nzval, diag_dev, nrows, n_own, index_base, theta, s_rowptr_dev,
                                            info_dev, work, stream);
}

HPCLA_API int hpcla_amg_strength_count_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                               const double *diag_dev, int64_t nrows, int64_t n_own, int index_base, double theta,
                                               int64_t *s_rowptr_dev, int64_t *info_dev, void *work, void *stream)
{
    return amg_strength_count_impl<int64_t>(rowptr, colval_split, nzval, diag_dev, nrows, n_own, index_base, theta, s_rowptr_dev,
                                            info_dev, work, stream);
}

HPCLA_API int hpcla_amg_strength_fill_f64_i32(const int32_t *rowptr, const int32_t *colval_split, const double *nzval,
                                              const double *diag_dev, int64_t nrows, int64_t n_own, int index_base, double theta,
                                              const int64_t *s_rowptr_dev, int32_t *s_cols_dev, void *stream)
{
    return amg_strength_fill_impl<int32_t>(rowptr, colval_split, nzval, diag_dev, nrows, n_own, index_base, theta, s_rowptr_dev,
                                           s_cols_dev, stream);
}

HPCLA_API int hpcla_amg_strength_fill_f64_i64(const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
                                              const double *diag_dev, int64_t nrows, int64_t n_own, int index_base, double theta,
                                              const int64_t *s_rowptr_dev, int32_t *s_cols_dev, void *stream)
{
    return amg_strength_fill_impl<int64_t>(rowptr, colval_split, nzval, diag_dev, nrows, n_own, index_base, theta, s_rowptr_dev,
                                           s_cols_dev, stream);
}

HPCLA_API int hpcla_amg_symmetrise_count(const int64_t *s_rowptr_dev, const int32_t *s_cols_dev, int64_t nrows, int64_t *indeg_dev,
                                         int64_t *u_rowptr_dev, int64_t *info_dev, void *work, void *stream)
{
    if (nrows < 0 || nrows > 0x7fffffffLL) return set_error(HPCLA_ERR_INVALID, "amg_symmetrise_count: needs 0 <= nrows < 2^31");
    if (!u_rowptr_dev || !info_dev || !work) return set_error(HPCLA_ERR_INVALID, "amg_symmetrise_count: null rowptr / info / work");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(info_dev, 0, sizeof(int64_t), s));
    if (nrows == 0) {
        HPCLA_CHECK_HIP(hipMemsetAsync(u_rowptr_dev, 0, sizeof(int64_t), s));
        return HPCLA_OK;
    }
    if (!s_rowptr_dev || !indeg_dev) return set_error(HPCLA_ERR_INVALID, "amg_symmetrise_count: null array");   // s_cols may be NULL
    HPCLA_CHECK_HIP(hipMemsetAsync(indeg_dev, 0, sizeof(int64_t) * (size_t)nrows, s));
    amg_indegree_kernel<<<amg_group_grid(nrows), AMG_THREADS, 0, s>>>(s_rowptr_dev, s_cols_dev, nrows, indeg_dev);
    HPCLA_CHECK_LAUNCH();
    int64_t *sums = reinterpret_cast<int64_t *>(work);
    return exclusive_scan(AmgDegreeLoad{s_rowptr_dev, indeg_dev}, nrows, AmgRowptrEmit{nrows, u_rowptr_dev, info_dev}, sums + 1, sums,
                          s);
}

HPCLA_API int hpcla_amg_symmetrise_fill(const int64_t *s_rowptr_dev, const int32_t *s_cols_dev, int64_t nrows,
                                        const int64_t *u_rowptr_dev, int64_t *cursor_dev, int32_t *u_cols_dev, void *stream)
{
    if (nrows < 0 || nrows > 0x7fffffffLL) return set_error(HPCLA_ERR_INVALID, "amg_symmetrise_fill: needs 0 <= nrows < 2^31");
    if (nrows == 0) return HPCLA_OK;
    if (!s_rowptr_dev || !u_rowptr_dev || !cursor_dev)
        return set_error(HPCLA_ERR_INVALID, "amg_symmetrise_fill: null array");            // both column arrays NULL: no edges
    hipStream_t s = as_stream(stream);
    amg_symmetrise_copy_kernel<<<amg_group_grid(nrows), AMG_THREADS, 0, s>>>(s_rowptr_dev, s_cols_dev, nrows, u_rowptr_dev,
                                                                            cursor_dev, u_cols_dev);
    HPCLA_CHECK_LAUNCH();
    amg_symmetrise_scatter_kernel<<<amg_group_grid(nrows), AMG_THREADS, 0, s>>>(s_rowptr_dev, s_cols_dev, nrows, u_rowptr_dev,
                                                                               cursor_dev, u_cols_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_amg_mis_init(int64_t nrows, int64_t row_start, int64_t *key_dev, int64_t *state_dev, void *stream)
{
    if (nrows < 0 || nrows > 0x7fffffffLL || row_start < 0)
        return set_error(HPCLA_ERR_INVALID, "amg_mis_init: needs 0 <= nrows < 2^31 and row_start >= 0");
    if (nrows == 0) return HPCLA_OK;
    if (!key_dev || !state_dev) return set_error(HPCLA_ERR_INVALID, "amg_mis_init: null array");
    amg_mis_init_kernel<<<amg_row_grid(nrows), AMG_THREADS, 0, as_stream(stream)>>>(nrows, row_start, key_dev, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_amg_mis_round(const int64_t *s_rowptr_dev, const int32_t *s_cols_dev, int64_t nrows, const int64_t *key_dev,
                                  const int64_t *state_in_dev, int64_t *m1_dev, int64_t *m2_dev, int64_t *state_out_dev,
                                  int64_t *block_undecided_dev, void *stream)
{
    if (nrows < 0 || nrows > 0x7fffffffLL) return set_error(HPCLA_ERR_INVALID, "amg_mis_round: needs 0 <= nrows < 2^31");
    if (!block_undecided_dev) return set_error(HPCLA_ERR_INVALID, "amg_mis_round: null counts");
    hipStream_t s = as_stream(stream);
    if (nrows == 0) {
        HPCLA_CHECK_HIP(hipMemsetAsync(block_undecided_dev, 0, sizeof(int64_t), s));
        return HPCLA_OK;
    }
    if (!s_rowptr_dev || !key_dev || !state_in_dev || !m1_dev || !m2_dev || !state_out_dev)
        return set_error(HPCLA_ERR_INVALID, "amg_mis_round: null array");     // s_cols may be NULL: a graph without edges
    amg_neighbour_max_kernel<<<amg_group_grid(nrows), AMG_THREADS, 0, s>>>(s_rowptr_dev, s_cols_dev, nrows, state_in_dev, m1_dev);
    HPCLA_CHECK_LAUNCH();
    amg_neighbour_max_kernel<<<amg_group_grid(nrows), AMG_THREADS, 0, s>>>(s_rowptr_dev, s_cols_dev, nrows, m1_dev, m2_dev);
    HPCLA_CHECK_LAUNCH();
    amg_mis_decide_kernel<<<amg_row_grid(nrows), AMG_THREADS, 0, s>>>(key_dev, m2_dev, state_in_dev, state_out_dev, nrows,
                                                                     block_undecided_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_amg_join(const int64_t *s_rowptr_dev, const int32_t *s_cols_dev, int64_t nrows, const int64_t *key_dev,
                             const int64_t *state_dev, int32_t *owner_a_dev, int32_t *owner_b_dev, int64_t *rootid_dev,
                             int64_t *info_dev, void *work, void *stream)
{
    if (nrows < 0 || nrows > 0x7fffffffLL) return set_error(HPCLA_ERR_INVALID, "amg_join: needs 0 <= nrows < 2^31");
    if (!info_dev || !work) return set_error(HPCLA_ERR_INVALID, "amg_join: null info / work");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(info_dev, 0xff, sizeof(int64_t), s));
    HPCLA_CHECK_HIP(hipMemsetAsync(info_dev + 1, 0, sizeof(int64_t), s));
    if (nrows == 0) return HPCLA_OK;
    if (!s_rowptr_dev || !key_dev || !state_dev || !owner_a_dev || !owner_b_dev || !rootid_dev)
        return set_error(HPCLA_ERR_INVALID, "amg_join: null array");
    amg_join_kernel<1><<<amg_group_grid(nrows), AMG_THREADS, 0, s>>>(s_rowptr_dev, s_cols_dev, nrows, key_dev, state_dev, nullptr,
                                                                    owner_a_dev, info_dev);
    HPCLA_CHECK_LAUNCH();
    amg_join_kernel<2><<<amg_group_grid(nrows), AMG_THREADS, 0, s>>>(s_rowptr_dev, s_cols_dev, nrows, key_dev, state_dev, owner_a_dev,
                                                                    owner_b_dev, info_dev);
    HPCLA_CHECK_LAUNCH();
    int64_t *sums = reinterpret_cast<int64_t *>(work);
    return exclusive_scan(AmgRootLoad{state_dev}, nrows, AmgRootEmit{nrows, rootid_dev, info_dev + 1}, sums + 1, sums, s);
}

HPCLA_API int hpcla_amg_aggregate_ids(const int32_t *owner_dev, const int64_t *rootid_dev, int64_t nrows, int64_t offset,
                                      int64_t *agg_dev, void *stream)
{
    if (nrows < 0 || nrows > 0x7fffffffLL || offset < 0)
        return set_error(HPCLA_ERR_INVALID, "amg_aggregate_ids: needs 0 <= nrows < 2^31 and offset >= 0");
    if (nrows == 0) return HPCLA_OK;
    if (!owner_dev || !rootid_dev || !agg_dev) return set_error(HPCLA_ERR_INVALID, "amg_aggregate_ids: null array");
    amg_ids_kernel<<<amg_row_grid(nrows), AMG_THREADS, 0, as_stream(stream)>>>(owner_dev, rootid_dev, nrows, offset, agg_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_amg_prolongator_f64_i32(const int32_t *at_rowptr, const int32_t *at_colval, const int64_t *at_col_indices_dev,
                                            const double *at_nzval, const int64_t *agg_dev, const double *s_dev, int64_t nrows,
                                            int index_base, double *p_nzval, void *stream)
{
    return amg_prolongator_impl<int32_t>(at_rowptr, at_colval, at_col_indices_dev, at_nzval, agg_dev, s_dev, nrows, index_base,
                                         p_nzval, stream);
}

HPCLA_API int hpcla_amg_prolongator_f64_i64(const int64_t *at_rowptr, const int64_t *at_colval, const int64_t *at_col_indices_dev,
                                            const double *at_nzval, const int64_t *agg_dev, const double *s_dev, int64_t nrows,
                                            int index_base, double *p_nzval, void *stream)
{
    return amg_prolongator_impl<int64_t>(at_rowptr, at_colval, at_col_indices_dev, at_nzval, agg_dev, s_dev, nrows, index_base,
                                         p_nzval, stream);
}

HPCLA_API int hpcla_amg_restrictor_f64_i32(const int32_t *ta_rowptr, const int32_t *ta_colval, const int64_t *ta_col_indices_dev,
                                           const double *ta_nzval, const int64_t *agg_dev, const double *s_dev, int64_t nrows,
                                           int64_t ncols, int64_t row_offset, int index_base, double *r_nzval, void *stream)
{
    return amg_restrictor_impl<int32_t>(ta_rowptr, ta_colval, ta_col_indices_dev, ta_nzval, agg_dev, s_dev, nrows, ncols, row_offset,
                                        index_base, r_nzval, stream);
}

HPCLA_API int hpcla_amg_restrictor_f64_i64(const int64_t *ta_rowptr, const int64_t *ta_colval, const int64_t *ta_col_indices_dev,
                                           const double *ta_nzval, const int64_t *agg_dev, const double *s_dev, int64_t nrows,
                                           int64_t ncols, int64_t row_offset, int index_base, double *r_nzval, void *stream)
{
    return amg_restrictor_impl<int64_t>(ta_rowptr, ta_colval, ta_col_indices_dev, ta_nzval, agg_dev, s_dev, nrows, ncols, row_offset,
                                        index_base, r_nzval, stream);
}

HPCLA_API int hpcla_amg_fit_f64(const double *b_dev, int64_t nrows, int k, const int64_t *member_ptr_dev, const int64_t *members_dev,
                                int64_t n_members, int64_t n_aggregates, double *tv_dev, double *bc_dev, int64_t *info_dev,
                                void *stream)
{
    if (nrows < 0 || n_members < 0 || n_aggregates < 0) return set_error(HPCLA_ERR_INVALID, "amg_fit: negative size");
    if (nrows > 0x7fffffffLL || n_aggregates > 0x7fffffffLL)
        return set_error(HPCLA_ERR_UNSUPPORTED, "amg_fit: at most 2^31 - 1 rows and aggregates per rank");
    if (k < 1 || k > AMG_G) return set_error(HPCLA_ERR_INVALID, "amg_fit: k must lie in 1..8");
    if (!info_dev) return set_error(HPCLA_ERR_INVALID, "amg_fit: null info");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(info_dev, 0xff, sizeof(int64_t), s));
    if (n_aggregates == 0) return HPCLA_OK;
    if (!member_ptr_dev || !tv_dev || !bc_dev || (n_members > 0 && (!b_dev || !members_dev)))
        return set_error(HPCLA_ERR_INVALID, "amg_fit: null array");
    if (b_dev == tv_dev) return set_error(HPCLA_ERR_INVALID, "amg_fit: B and Tv must be two arrays");
    HPCLA_CHECK_GRID((n_aggregates * AMG_G + AMG_THREADS - 1) / AMG_THREADS, "amg_fit");
    switch (k) {
    case 1: amg_fit_launch<1>(b_dev, nrows, member_ptr_dev, members_dev, n_members, n_aggregates, tv_dev, bc_dev, info_dev, s); break;
    case 2: amg_fit_launch<2>(b_dev, nrows, member_ptr_dev, members_dev, n_members, n_aggregates, tv_dev, bc_dev, info_dev, s); break;
    case 3: amg_fit_launch<3>(b_dev, nrows, member_ptr_dev, members_dev, n_members, n_aggregates, tv_dev, bc_dev, info_dev, s); break;
    case 4: amg_fit_launch<4>(b_dev, nrows, member_ptr_dev, members_dev, n_members, n_aggregates, tv_dev, bc_dev, info_dev, s); break;
    case 5: amg_fit_launch<5>(b_dev, nrows, member_ptr_dev, members_dev, n_members, n_aggregates, tv_dev, bc_dev, info_dev, s); break;
    case 6: amg_fit_launch<6>(b_dev, nrows, member_ptr_dev, members_dev, n_members, n_aggregates, tv_dev, bc_dev, info_dev, s); break;
    case 7: amg_fit_launch<7>(b_dev, nrows, member_ptr_dev, members_dev, n_members, n_aggregates, tv_dev, bc_dev, info_dev, s); break;
    default: amg_fit_launch<8>(b_dev, nrows, member_ptr_dev, members_dev, n_members, n_aggregates, tv_dev, bc_dev, info_dev, s); break;
    }
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_amg_prolongator_b_f64_i32(const int32_t *at_rowptr, const int32_t *at_colval, const int64_t *at_col_indices_dev,
                                              const double *at_nzval, const int64_t *agg_dev, const double *s_dev,
                                              const double *tv_dev, int k, int64_t nrows, int index_base, double *p_nzval,
                                              void *stream)
{
    return amg_prolongator_b_impl<int32_t>(at_rowptr, at_colval, at_col_indices_dev, at_nzval, agg_dev, s_dev, tv_dev, k, nrows,
                                           index_base, p_nzval, stream);
}

HPCLA_API int hpcla_amg_prolongator_b_f64_i64(const int64_t *at_rowptr, const int64_t *at_colval, const int64_t *at_col_indices_dev,
                                              const double *at_nzval, const int64_t *agg_dev, const double *s_dev,
                                              const double *tv_dev, int k, int64_t nrows, int index_base, double *p_nzval,
                                              void *stream)
{
    return amg_prolongator_b_impl<int64_t>(at_rowptr, at_colval, at_col_indices_dev, at_nzval, agg_dev, s_dev, tv_dev, k, nrows,
                                           index_base, p_nzval, stream);
}

HPCLA_API int hpcla_amg_restrictor_b_f64_i32(const int32_t *ta_rowptr, const int32_t *ta_colval, const int64_t *ta_col_indices_dev,
                                             const double *ta_nzval, const int64_t *agg_dev, const double *s_dev,
                                             const double *tv_dev, int k, int64_t nrows, int64_t ncols, int64_t row_offset,
                                             int index_base, double *r_nzval, void *stream)
{
    return amg_restrictor_b_impl<int32_t>(ta_rowptr, ta_colval, ta_col_indices_dev, ta_nzval, agg_dev, s_dev, tv_dev, k, nrows, ncols,
                                          row_offset, index_base, r_nzval, stream);
}

HPCLA_API int hpcla_amg_restrictor_b_f64_i64(const int64_t *ta_rowptr, const int64_t *ta_colval, const int64_t *ta_col_indices_dev,
                                             const double *ta_nzval, const int64_t *agg_dev, const double *s_dev,
                                             const double *tv_dev, int k, int64_t nrows, int64_t ncols, int64_t row_offset,
                                             int index_base, double *r_nzval, void *stream)
{
    return amg_restrictor_b_impl<int64_t>(ta_rowptr, ta_colval, ta_col_indices_dev, ta_nzval, agg_dev, s_dev, tv_dev, k, nrows, ncols,
                                          row_offset, index_base, r_nzval, stream);
}

HPCLA_API int hpcla_amg_presmooth_f64(const double *s_dev, const double *b, double *x, int64_t n, void *stream)
{
    return amg_smooth_impl<0>(s_dev, b, nullptr, x, n, stream);
}

HPCLA_API int hpcla_amg_postsmooth_f64(const double *s_dev, const double *b, const double *t, double *x, int64_t n, void *stream)
{
    return amg_smooth_impl<1>(s_dev, b, t, x, n, stream);
}
