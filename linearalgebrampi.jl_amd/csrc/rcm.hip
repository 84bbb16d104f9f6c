// rcm.hip -- the reverse Cuthill-McKee ordering of a rank's owned block (hp.rcm) and the bandwidth of a matrix (hp.bandwidth).
//
// The graph.  Rows and columns of A are partitioned alike, so a stored entry whose global column lies in this rank's row range
// names a local row; every other entry is dropped, and so is the diagonal.  The owned block's off-diagonal pattern becomes a CSR
// of its own: g_rowptr (int64, nrows + 1, 0-based) by the library's scan (scan.h), g_cols (int32 local columns, stored order
// kept).  A's compressed columns are read through its global column ids, so neither a plan nor a hash of A is needed.  For a
// nonsymmetric pattern the caller passes the graph through hpcla_amg_symmetrise_count / _fill, which may list a neighbour
// twice: deg[] then counts the DISTINCT neighbours (rcm_degree_kernel, distinct != 0), and a repeated neighbour is harmless to
// the walk (the second atomic min changes nothing).
//
// The ordering (tests/_rcm_cases.py restates it in numpy).  by_degree = the vertices sorted by (deg, index), rank = its inverse.
// Vertices without a neighbour take the numbers 0 .. z - 1 (they sort first).  While unnumbered vertices remain, the first
// unnumbered vertex of by_degree starts a component and takes the next number; level by level every unnumbered neighbour u of a
// level vertex gets parent[u] = the smallest number among the level vertices that list it, and the new vertices are numbered
// in ascending order of the key (parent[u] << 32) | rank[u].  p reverses the numbering.
//
// One state array.  parent[v] (int32) is RCM_UNVISITED until v is claimed and is touched through agent-scope atomics only: an
// atomic min that returns the old value claims (the lane that sees RCM_UNVISITED appends u to the level's candidates, exactly
// once per vertex), a vertex numbered earlier holds a parent below the current level's first number and is left alone.  No
// kernel reads with a plain load a word that the same launch wrote: parent is read back by relaxed agent-scope atomic loads.
//
// Two ways to walk a level, with the same result element for element:
//   wide    one level per call, any size: rcm_expand_kernel (a group of RCM_G lanes per frontier vertex and chunk of
//           RCM_CHUNK neighbours, so a long row is spread over many groups; candidates appended through one counter, one
//           atomic add per wave), rcm_keys_kernel once the expand has finished, the caller's sort, rcm_number_kernel.
//   narrow  rcm_narrow_kernel: ONE workgroup walks level after level while the frontier has at most RCM_FRONTIER_CAP
//           vertices and the sum of its row lengths is at most RCM_CANDIDATE_CAP (tested by a reduction before parent is
//           touched: a level is never half done).  Frontier and keys live in LDS, the sort is a bitonic network there, and a
//           component that ends is followed by the next start, found by scanning by_degree from a cursor.  The kernel uses
//           its own barrier only and waits on nothing else; it leaves (lo, hi, cursor, status, levels, starts) in a record.
#include "common.h"
#include "scan.h"

namespace hpcla {

constexpr int RCM_THREADS = 256;
constexpr int RCM_G = 8;                              // lanes per frontier vertex of the wide expand
constexpr int RCM_CHUNK = 256;                        // neighbours a group walks per chunk
constexpr int RCM_NARROW_THREADS = 1024;
constexpr int RCM_FRONTIER_CAP = 4096;
constexpr int RCM_CANDIDATE_CAP = 8192;
constexpr int RCM_ITEMS = RCM_FRONTIER_CAP / RCM_NARROW_THREADS;
constexpr int32_t RCM_UNVISITED = 0x7fffffff;
constexpr int RCM_DONE = 0, RCM_WIDE = 1, RCM_STUCK = 2;
// LDS of the narrow kernel: keys, frontier, offsets (+ 1, padded), 64 words of scalars and wave sums
constexpr size_t RCM_LDS_KEYS = (size_t)RCM_CANDIDATE_CAP * 8;
constexpr size_t RCM_LDS_FRONT = (size_t)RCM_FRONTIER_CAP * 4;
constexpr size_t RCM_LDS_OFF = (size_t)(RCM_FRONTIER_CAP + 16) * 4;
constexpr size_t RCM_LDS_BYTES = RCM_LDS_KEYS + RCM_LDS_FRONT + RCM_LDS_OFF + 64 * 4;

static inline uint32_t rcm_grid(int64_t n) { return (uint32_t)((n + RCM_THREADS - 1) / RCM_THREADS); }

__device__ __forceinline__ int32_t rcm_parent_of(int32_t *parent, int64_t v)
{
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the graph ------------------------------------------------------------------------------------------------------------------
template <typename I>
__device__ __forceinline__ int64_t rcm_local_column(const I *__restrict__ colval, const int64_t *__restrict__ col_indices, int64_t e,
                                                    int base, int64_t row_start)
{
    return col_indices[(int64_t)colval[e] - base] - base - row_start;
}

template <typename I>
struct RcmCountLoad {
    const I *rowptr, *colval;
    const int64_t *col_indices;
    int base;
    int64_t row_start, nrows;
    __device__ int64_t operator()(int64_t i) const
    {
        const int64_t e0 = (int64_t)rowptr[i] - base, e1 = (int64_t)rowptr[i + 1] - base;
        int64_t m = 0;
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t c = rcm_local_column(colval, col_indices, e, base, row_start);
            m += (c >= 0 && c < nrows && c != i) ? 1 : 0;
        }
        return m;
    }
};

struct RcmRowptrEmit {
    int64_t nrows;
    int64_t *g_rowptr, *total;
    __device__ void operator()(int64_t i, int64_t before, int64_t m) const
    {
        g_rowptr[i] = before;
        if (i == nrows - 1) {
            g_rowptr[nrows] = before + m;
            total[0] = before + m;
        }
    }
};

template <typename I>
__global__ __launch_bounds__(RCM_THREADS) void rcm_graph_fill_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                     const int64_t *__restrict__ col_indices, int64_t nrows,
                                                                     int64_t row_start, int base,
                                                                     const int64_t *__restrict__ g_rowptr,
                                                                     int32_t *__restrict__ g_cols)
{
    const int64_t i = (int64_t)blockIdx.x * RCM_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int64_t e0 = (int64_t)rowptr[i] - base, e1 = (int64_t)rowptr[i + 1] - base;
    int64_t pos = g_rowptr[i];
    const int64_t end = g_rowptr[i + 1];
    for (int64_t e = e0; e < e1; ++e) {
        const int64_t c = rcm_local_column(colval, col_indices, e, base, row_start);
        if (c >= 0 && c < nrows && c != i && pos < end) g_cols[pos++] = (int32_t)c;
    }
}

// deg[i] = the entries of row i, or -- distinct -- those that no earlier entry of the row repeats; RCM_G lanes per row
__global__ __launch_bounds__(RCM_THREADS) void rcm_degree_kernel(const int64_t *__restrict__ g_rowptr,
                                                                 const int32_t *__restrict__ g_cols, int64_t nrows, int distinct,
                                                                 int32_t *__restrict__ deg)
{
    const int64_t i = ((int64_t)blockIdx.x * RCM_THREADS + threadIdx.x) / RCM_G;
    const int l = threadIdx.x & (RCM_G - 1);
    const bool live = i < nrows;
    int32_t m = 0;
    if (live) {
        const int64_t e0 = g_rowptr[i], e1 = g_rowptr[i + 1];
        if (!distinct) {
            m = l == 0 ? (int32_t)(e1 - e0) : 0;
        } else {
            for (int64_t e = e0 + l; e < e1; e += RCM_G) {
                const int32_t c = g_cols[e];
                bool first = true;
                for (int64_t e2 = e0; e2 < e && first; ++e2) first = g_cols[e2] != c;
                m += first ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int off = RCM_G / 2; off > 0; off >>= 1) m += __shfl_xor(m, off, RCM_G);
    if (live && l == 0) deg[i] = m;
}

// rank = the inverse of by_degree; parent = unvisited; the vertices without a neighbour take 0 .. z - 1; info[0] = z when z > 0
__global__ __launch_bounds__(RCM_THREADS) void rcm_init_kernel(const int32_t *__restrict__ deg, const int32_t *__restrict__ by_degree,
                                                               int64_t nrows, int32_t *__restrict__ rank,
                                                               int32_t *__restrict__ parent, int32_t *__restrict__ order,
                                                               int64_t *__restrict__ info)
{
    const int64_t i = (int64_t)blockIdx.x * RCM_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int32_t v = by_degree[i];
    if (v < 0 || v >= nrows) return;
    rank[v] = (int32_t)i;
    if (deg[v] == 0) {
        order[i] = v;
        parent[v] = (int32_t)i;
        bool last = i == nrows - 1;
        if (!last) {
            const int32_t w = by_degree[i + 1];
            last = w >= 0 && w < nrows && deg[w] != 0;
        }
        if (last) info[0] = i + 1;
    } else {
        parent[v] = RCM_UNVISITED;
    }
}

// ---- a wide level ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RCM_THREADS) void rcm_expand_kernel(const int64_t *__restrict__ g_rowptr,
                                                                 const int32_t *__restrict__ g_cols, int64_t nrows,
                                                                 const int32_t *__restrict__ order, int64_t lo, int64_t f,
                                                                 int64_t nchunks, int32_t *__restrict__ parent,
                                                                 int32_t *__restrict__ cand, unsigned long long *__restrict__ count)
{
    const int64_t grp = ((int64_t)blockIdx.x * RCM_THREADS + threadIdx.x) / RCM_G;
    const int l = threadIdx.x & (RCM_G - 1);
    const int lane = threadIdx.x & 63;
    const bool live = grp < f;
    int64_t r0 = 0, r1 = 0;
    int32_t num = 0;
    if (live) {
        const int32_t v = order[lo + grp];
        if (v >= 0 && v < nrows) {
            r0 = g_rowptr[v];
            r1 = g_rowptr[v + 1];
        }
        num = (int32_t)(lo + grp);
    }
    for (int64_t chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
        const int64_t e0 = r0 + chunk * RCM_CHUNK;
        for (int it = 0; it < RCM_CHUNK / RCM_G; ++it) {
            const int64_t e = e0 + it * RCM_G + l;
            const bool valid = live && e < r1;
            if (!__any(valid)) break;
            bool claimed = false;
            int32_t u = 0;
            if (valid) {
                u = g_cols[e];
                if (u >= 0 && u < nrows) claimed = atomicMin(parent + u, num) == RCM_UNVISITED;
            }
            const unsigned long long mask = __ballot(claimed);
            if (mask) {                                              // one atomic per wave
                const int leader = __ffsll((long long)mask) - 1;
                unsigned long long base = 0;
                if (lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(mask));
                base = __shfl(base, leader, 64);
                if (claimed) {
                    const unsigned long long pos = base + __popcll(mask & ((1ULL << lane) - 1ULL));
                    if (pos < (unsigned long long)nrows) cand[pos] = u;
                }
            }
        }
    }
}

__global__ __launch_bounds__(RCM_THREADS) void rcm_keys_kernel(const int32_t *__restrict__ cand, int64_t ncand, int64_t nrows,
                                                               int32_t *__restrict__ parent, const int32_t *__restrict__ rank,
                                                               int64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * RCM_THREADS + threadIdx.x;
    if (i >= ncand) return;
    const int32_t u = cand[i];
    if (u < 0 || u >= nrows) {
        keys[i] = 0;
        return;
    }
    keys[i] = ((int64_t)rcm_parent_of(parent, u) << 32) | (int64_t)(uint32_t)rank[u];
}

__global__ __launch_bounds__(RCM_THREADS) void rcm_number_kernel(const int64_t *__restrict__ keys, int64_t ncand, int64_t nrows,
                                                                 const int32_t *__restrict__ by_degree, int64_t cnt,
                                                                 int32_t *__restrict__ order)
{
    const int64_t i = (int64_t)blockIdx.x * RCM_THREADS + threadIdx.x;
    if (i >= ncand || cnt + i >= nrows) return;
    const int64_t r = keys[i] & 0xffffffffLL;
    if (r < nrows) order[cnt + i] = by_degree[r];
}

// ---- narrow levels: one workgroup ------------------------------------------------------------------------------------------------
// s[0 .. 15] wave sums, s[16] the found start, s[17] the candidate count, s[18] what the start's claim returned
__global__ __launch_bounds__(RCM_NARROW_THREADS) void rcm_narrow_kernel(
    const int64_t *__restrict__ g_rowptr, const int32_t *__restrict__ g_cols, const int32_t *__restrict__ by_degree,
    const int32_t *__restrict__ rank, int32_t n, int32_t lo, int32_t hi, int32_t cursor, const int64_t *__restrict__ first,
    int32_t *__restrict__ parent, int32_t *__restrict__ order, int64_t *__restrict__ record)
{
    extern __shared__ __attribute__((aligned(16))) char rcm_smem[];
    unsigned long long *s_keys = reinterpret_cast<unsigned long long *>(rcm_smem);
    int32_t *s_front = reinterpret_cast<int32_t *>(rcm_smem + RCM_LDS_KEYS);
    int32_t *s_off = reinterpret_cast<int32_t *>(rcm_smem + RCM_LDS_KEYS + RCM_LDS_FRONT);
    int32_t *s = reinterpret_cast<int32_t *>(rcm_smem + RCM_LDS_KEYS + RCM_LDS_FRONT + RCM_LDS_OFF);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (first) lo = hi = cursor = (int32_t)first[0];
    int32_t levels = 0, starts = 0, status;
    bool loaded = false;                                      // the frontier order[lo .. hi) is in s_front
    // every branch below is taken by the whole workgroup: lo, hi, cursor and what is read from LDS behind a barrier are uniform
    for (;;) {
        int32_t f = hi - lo;
        if (f == 0) {                                         // a component ended (or none has begun): the next start
            if (hi >= n) {
                status = RCM_DONE;
                break;
            }
            int32_t found = RCM_UNVISITED;
            while (cursor < n) {
                if (tid == 0) s[16] = RCM_UNVISITED;
                __syncthreads();
                const int32_t i = cursor + tid;
                if (i < n) {
                    const int32_t bv = by_degree[i];
                    if (bv >= 0 && bv < n && rcm_parent_of(parent, bv) == RCM_UNVISITED) atomicMin(&s[16], i);
                }
                __syncthreads();
                found = s[16];
                __syncthreads();
                if (found != RCM_UNVISITED) break;
                cursor += RCM_NARROW_THREADS;
            }
            if (found == RCM_UNVISITED) {                     // hi < n and nothing unnumbered: not reachable
                status = RCM_STUCK;
                break;
            }
            cursor = found + 1;
            if (tid == 0) {                                   // the returned value is used, so the claim has landed at the barrier
                const int32_t sv = by_degree[found];
                s[18] = atomicMin(parent + sv, hi);
                order[hi] = sv;
                s_front[0] = sv;
            }
            lo = hi;
            hi = hi + 1;
            f = 1;
            loaded = true;
            ++starts;
            ++levels;
            __syncthreads();
        }
        if (f > RCM_FRONTIER_CAP) {
            status = RCM_WIDE;
            break;
        }
        if (!loaded) {                                        // written by an earlier launch
            for (int32_t j = tid; j < f; j += RCM_NARROW_THREADS) s_front[j] = order[lo + j];
            loaded = true;
            __syncthreads();
        }
        // the exclusive scan of the frontier's row lengths (each clamped to the cap + 1, so the sum stays small)
        int32_t d[RCM_ITEMS], mine = 0;
#pragma unroll
        for (int k = 0; k < RCM_ITEMS; ++k) {
            const int32_t j = tid * RCM_ITEMS + k;
            d[k] = 0;
            if (j < f) {
                const int32_t v = s_front[j];
                const int64_t len = g_rowptr[v + 1] - g_rowptr[v];
                d[k] = len > RCM_CANDIDATE_CAP ? RCM_CANDIDATE_CAP + 1 : (int32_t)len;
            }
            mine += d[k];
        }
        int32_t inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t t = __shfl_up(inc, off, 64);
            if (lane >= off) inc += t;
        }
        if (lane == 63) s[w] = inc;
        __syncthreads();
        int32_t before = inc - mine, total = 0;
        for (int k = 0; k < RCM_NARROW_THREADS / 64; ++k) {
            if (k < w) before += s[k];
            total += s[k];
        }
#pragma unroll
        for (int k = 0; k < RCM_ITEMS; ++k) {
            const int32_t j = tid * RCM_ITEMS + k;
            if (j < f) s_off[j] = before;
            before += d[k];
        }
        if (tid == 0) {
            s_off[f] = total;
            s[17] = 0;
        }
        __syncthreads();
        if (total > RCM_CANDIDATE_CAP) {                      // parent is untouched: the level goes to the wide path whole
            status = RCM_WIDE;
            break;
        }
        // expand: one lane per edge of the level
        for (int32_t e = tid; e < total; e += RCM_NARROW_THREADS) {
            int32_t a = 0, b = f;                             // the last j with s_off[j] <= e (an empty row never wins)
            while (b - a > 1) {
                const int32_t m = (a + b) >> 1;
                if (s_off[m] <= e) a = m; else b = m;
            }
            const int32_t v = s_front[a];
            const int32_t u = g_cols[g_rowptr[v] + (e - s_off[a])];
            if (u >= 0 && u < n && atomicMin(parent + u, lo + a) == RCM_UNVISITED) {
                const int32_t pos = atomicAdd(&s[17], 1);
                if (pos < RCM_CANDIDATE_CAP) s_keys[pos] = (unsigned long long)(uint32_t)u;
            }
        }
        __syncthreads();
        const int32_t ncand = s[17] < RCM_CANDIDATE_CAP ? s[17] : RCM_CANDIDATE_CAP;
        if (ncand == 0) {                                     // the component is complete
            lo = hi;
            continue;
        }
        int32_t m = 1;
        while (m < ncand) m <<= 1;
        for (int32_t i = tid; i < m; i += RCM_NARROW_THREADS) {
            if (i < ncand) {
                const uint32_t u = (uint32_t)s_keys[i];
                s_keys[i] = ((unsigned long long)(uint32_t)rcm_parent_of(parent, u) << 32) | (uint32_t)rank[u];
            } else {
                s_keys[i] = ~0ULL;
            }
        }
        __syncthreads();
        for (int32_t k = 2; k <= m; k <<= 1) {                // bitonic network, ascending
            for (int32_t j = k >> 1; j > 0; j >>= 1) {
                for (int32_t t = tid; t < (m >> 1); t += RCM_NARROW_THREADS) {
                    const int32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const int32_t p = i | j;
                    const unsigned long long x = s_keys[i], y = s_keys[p];
                    const bool up = (i & k) == 0;
                    if ((x > y) == up) {
                        s_keys[i] = y;
                        s_keys[p] = x;
                    }
                }
                __syncthreads();
            }
        }
        for (int32_t i = tid; i < ncand; i += RCM_NARROW_THREADS) {
            const uint32_t r = (uint32_t)s_keys[i];
            const int32_t u = r < (uint32_t)n ? by_degree[r] : 0;
            if (hi + i < n) order[hi + i] = u;
            if (i < RCM_FRONTIER_CAP) s_front[i] = u;
        }
        lo = hi;
        hi += ncand;
        ++levels;
        __syncthreads();
    }
    if (tid == 0) {
        record[0] = lo;
        record[1] = hi;
        record[2] = cursor;
        record[3] = status;
        record[4] = levels;
        record[5] = starts;
    }
}

// ---- finish ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RCM_THREADS) void rcm_finish_kernel(const int32_t *__restrict__ order, int64_t nrows, int64_t row_start,
                                                                 int64_t *__restrict__ p, int32_t *__restrict__ inv)
{
    const int64_t i = (int64_t)blockIdx.x * RCM_THREADS + threadIdx.x;
    if (i >= nrows) return;
    const int32_t v = order[nrows - 1 - i];
    p[i] = (int64_t)v + row_start;
    if (v >= 0 && v < nrows) inv[v] = (int32_t)i;
}

// the workgroup's maximum, then one atomic
__device__ __forceinline__ void rcm_block_max(int64_t m, unsigned long long *out)
{
    __shared__ int64_t s_max[RCM_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t t = __shfl_xor(m, off, 64);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < RCM_THREADS / 64; ++k) m = s_max[k] > m ? s_max[k] : m;
        if (m > 0) atomicMax(out, (unsigned long long)m);
    }
}

// max |inv[i] - inv[c]| over the graph (inv == NULL: |i - c|)
__global__ __launch_bounds__(RCM_THREADS) void rcm_graph_bandwidth_kernel(const int64_t *__restrict__ g_rowptr,
                                                                          const int32_t *__restrict__ g_cols, int64_t nrows,
                                                                          const int32_t *__restrict__ inv,
                                                                          unsigned long long *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * RCM_THREADS + threadIdx.x;
    int64_t m = 0;
    if (i < nrows) {
        const int64_t a = inv ? inv[i] : i;
        for (int64_t e = g_rowptr[i]; e < g_rowptr[i + 1]; ++e) {
            const int64_t c = g_cols[e];
            if (c < 0 || c >= nrows) continue;
            const int64_t dlt = a - (inv ? (int64_t)inv[c] : c);
            m = (dlt < 0 ? -dlt : dlt) > m ? (dlt < 0 ? -dlt : dlt) : m;
        }
    }
    rcm_block_max(m, out);
}

// max |row_start + i - global column| over every stored entry of the rank's rows
template <typename I>
__global__ __launch_bounds__(RCM_THREADS) void rcm_matrix_bandwidth_kernel(const I *__restrict__ rowptr, const I *__restrict__ colval,
                                                                           const int64_t *__restrict__ col_indices, int64_t nrows,
                                                                           int64_t row_start, int base,
                                                                           unsigned long long *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * RCM_THREADS + threadIdx.x;
    int64_t m = 0;
    if (i < nrows) {
        const int64_t e0 = (int64_t)rowptr[i] - base, e1 = (int64_t)rowptr[i + 1] - base;
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t dlt = rcm_local_column(colval, col_indices, e, base, row_start) - i;
            m = (dlt < 0 ? -dlt : dlt) > m ? (dlt < 0 ? -dlt : dlt) : m;
        }
    }
    rcm_block_max(m, out);
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
static int rcm_check_rows(int64_t nrows, const char *what)
{
    if (nrows < 0) return set_error(HPCLA_ERR_INVALID, "%s: negative size", what);
    if (nrows >= 0x7fffffffLL) return set_error(HPCLA_ERR_UNSUPPORTED, "%s: needs nrows < 2^31 - 1", what);
    return HPCLA_OK;
}

template <typename I>
static int rcm_graph_count_impl(const I *rowptr, const I *colval, const int64_t *col_indices, int64_t nrows, int64_t row_start,
                                int index_base, int64_t *g_rowptr, int64_t *info, void *work, void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_graph_count")) return st;
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "rcm_graph_count: index_base must be 0 or 1");
    if (!g_rowptr || !info || !work) return set_error(HPCLA_ERR_INVALID, "rcm_graph_count: null rowptr / info / work");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(info, 0, sizeof(int64_t), s));
    if (nrows == 0) {
        HPCLA_CHECK_HIP(hipMemsetAsync(g_rowptr, 0, sizeof(int64_t), s));
        return HPCLA_OK;
    }
    if (!rowptr) return set_error(HPCLA_ERR_INVALID, "rcm_graph_count: null CSR array");   // colval, col_indices: NULL when empty
    int64_t *sums = reinterpret_cast<int64_t *>(work);
    return exclusive_scan(RcmCountLoad<I>{rowptr, colval, col_indices, index_base, row_start, nrows}, nrows,
                          RcmRowptrEmit{nrows, g_rowptr, info}, sums + 1, sums, s);
}

template <typename I>
static int rcm_graph_fill_impl(const I *rowptr, const I *colval, const int64_t *col_indices, int64_t nrows, int64_t row_start,
                               int index_base, const int64_t *g_rowptr, int32_t *g_cols, void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_graph_fill")) return st;
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "rcm_graph_fill: index_base must be 0 or 1");
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr || !g_rowptr) return set_error(HPCLA_ERR_INVALID, "rcm_graph_fill: null array");
    rcm_graph_fill_kernel<I><<<rcm_grid(nrows), RCM_THREADS, 0, as_stream(stream)>>>(rowptr, colval, col_indices, nrows, row_start,
                                                                                    index_base, g_rowptr, g_cols);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

template <typename I>
static int rcm_matrix_bandwidth_impl(const I *rowptr, const I *colval, const int64_t *col_indices, int64_t nrows, int64_t row_start,
                                     int index_base, int64_t *out, void *stream)
{
    if (nrows < 0) return set_error(HPCLA_ERR_INVALID, "bandwidth: negative size");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "bandwidth: index_base must be 0 or 1");
    if (!out) return set_error(HPCLA_ERR_INVALID, "bandwidth: null result");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(int64_t), s));
    if (nrows == 0) return HPCLA_OK;
    if (!rowptr) return set_error(HPCLA_ERR_INVALID, "bandwidth: null CSR array");
    HPCLA_CHECK_GRID((nrows + RCM_THREADS - 1) / RCM_THREADS, "bandwidth");
    rcm_matrix_bandwidth_kernel<I><<<rcm_grid(nrows), RCM_THREADS, 0, s>>>(rowptr, colval, col_indices, nrows, row_start, index_base,
                                                                          reinterpret_cast<unsigned long long *>(out));
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_rcm_frontier_cap(void) { return RCM_FRONTIER_CAP; }

HPCLA_API int64_t hpcla_rcm_candidate_cap(void) { return RCM_CANDIDATE_CAP; }

HPCLA_API int64_t hpcla_rcm_work_bytes(int64_t nrows)
{
    if (nrows < 0) return -1;
    return (int64_t)sizeof(int64_t) * (1 + scan_blocks(nrows > 0 ? nrows : 1));
}

HPCLA_API int hpcla_rcm_graph_count_i32(const int32_t *rowptr, const int32_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                                        int64_t row_start, int index_base, int64_t *g_rowptr_dev, int64_t *info_dev, void *work,
                                        void *stream)
{
    return rcm_graph_count_impl<int32_t>(rowptr, colval, col_indices_dev, nrows, row_start, index_base, g_rowptr_dev, info_dev, work,
                                         stream);
}

HPCLA_API int hpcla_rcm_graph_count_i64(const int64_t *rowptr, const int64_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                                        int64_t row_start, int index_base, int64_t *g_rowptr_dev, int64_t *info_dev, void *work,
                                        void *stream)
{
    return rcm_graph_count_impl<int64_t>(rowptr, colval, col_indices_dev, nrows, row_start, index_base, g_rowptr_dev, info_dev, work,
                                         stream);
}

HPCLA_API int hpcla_rcm_graph_fill_i32(const int32_t *rowptr, const int32_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                                       int64_t row_start, int index_base, const int64_t *g_rowptr_dev, int32_t *g_cols_dev,
                                       void *stream)
{
    return rcm_graph_fill_impl<int32_t>(rowptr, colval, col_indices_dev, nrows, row_start, index_base, g_rowptr_dev, g_cols_dev, stream);
}

HPCLA_API int hpcla_rcm_graph_fill_i64(const int64_t *rowptr, const int64_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                                       int64_t row_start, int index_base, const int64_t *g_rowptr_dev, int32_t *g_cols_dev,
                                       void *stream)
{
    return rcm_graph_fill_impl<int64_t>(rowptr, colval, col_indices_dev, nrows, row_start, index_base, g_rowptr_dev, g_cols_dev, stream);
}

HPCLA_API int hpcla_rcm_degrees(const int64_t *g_rowptr_dev, const int32_t *g_cols_dev, int64_t nrows, int distinct, int32_t *deg_dev,
                                void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_degrees")) return st;
    if (nrows == 0) return HPCLA_OK;
    if (!g_rowptr_dev || !deg_dev) return set_error(HPCLA_ERR_INVALID, "rcm_degrees: null array");
    rcm_degree_kernel<<<rcm_grid(nrows * RCM_G), RCM_THREADS, 0, as_stream(stream)>>>(g_rowptr_dev, g_cols_dev, nrows, distinct,
                                                                                     deg_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_rcm_init(const int32_t *deg_dev, const int32_t *by_degree_dev, int64_t nrows, int32_t *rank_dev,
                             int32_t *parent_dev, int32_t *order_dev, int64_t *info_dev, void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_init")) return st;
    if (!info_dev) return set_error(HPCLA_ERR_INVALID, "rcm_init: null info");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(info_dev, 0, sizeof(int64_t), s));
    if (nrows == 0) return HPCLA_OK;
    if (!deg_dev || !by_degree_dev || !rank_dev || !parent_dev || !order_dev)
        return set_error(HPCLA_ERR_INVALID, "rcm_init: null array");
    rcm_init_kernel<<<rcm_grid(nrows), RCM_THREADS, 0, s>>>(deg_dev, by_degree_dev, nrows, rank_dev, parent_dev, order_dev, info_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_rcm_narrow(const int64_t *g_rowptr_dev, const int32_t *g_cols_dev, const int32_t *by_degree_dev,
                               const int32_t *rank_dev, int64_t nrows, int64_t lo, int64_t hi, int64_t cursor,
                               const int64_t *first_dev, int32_t *parent_dev, int32_t *order_dev, int64_t *record_dev, void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_narrow")) return st;
    if (!record_dev) return set_error(HPCLA_ERR_INVALID, "rcm_narrow: null record");
    if (!first_dev && (lo < 0 || lo > hi || hi > nrows || cursor < 0 || cursor > nrows))
        return set_error(HPCLA_ERR_INVALID, "rcm_narrow: needs 0 <= lo <= hi <= nrows and 0 <= cursor <= nrows");
    if (nrows > 0 && (!g_rowptr_dev || !by_degree_dev || !rank_dev || !parent_dev || !order_dev))
        return set_error(HPCLA_ERR_INVALID, "rcm_narrow: null array");                    // g_cols: NULL for a graph without edges
    HPCLA_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(rcm_narrow_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)RCM_LDS_BYTES));
    rcm_narrow_kernel<<<1, RCM_NARROW_THREADS, RCM_LDS_BYTES, as_stream(stream)>>>(
        g_rowptr_dev, g_cols_dev, by_degree_dev, rank_dev, (int32_t)nrows, (int32_t)lo, (int32_t)hi, (int32_t)cursor, first_dev,
        parent_dev, order_dev, record_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_rcm_expand(const int64_t *g_rowptr_dev, const int32_t *g_cols_dev, int64_t nrows, const int32_t *order_dev,
                               int64_t lo, int64_t hi, int64_t longest_row, int32_t *parent_dev, int32_t *cand_dev,
                               int64_t *count_dev, void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_expand")) return st;
    if (lo < 0 || lo > hi || hi > nrows || longest_row < 0)
        return set_error(HPCLA_ERR_INVALID, "rcm_expand: needs 0 <= lo <= hi <= nrows and longest_row >= 0");
    if (!count_dev) return set_error(HPCLA_ERR_INVALID, "rcm_expand: null count");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(count_dev, 0, sizeof(int64_t), s));
    if (hi == lo || longest_row == 0) return HPCLA_OK;
    if (!g_rowptr_dev || !g_cols_dev || !order_dev || !parent_dev || !cand_dev)
        return set_error(HPCLA_ERR_INVALID, "rcm_expand: null array");
    const int64_t nchunks = (longest_row + RCM_CHUNK - 1) / RCM_CHUNK;
    const int64_t gx = ((hi - lo) * RCM_G + RCM_THREADS - 1) / RCM_THREADS;
    HPCLA_CHECK_GRID(gx, "rcm_expand");
    const dim3 grid((uint32_t)gx, (uint32_t)(nchunks < 1024 ? nchunks : 1024));
    rcm_expand_kernel<<<grid, RCM_THREADS, 0, s>>>(g_rowptr_dev, g_cols_dev, nrows, order_dev, lo, hi - lo, nchunks, parent_dev,
                                                   cand_dev, reinterpret_cast<unsigned long long *>(count_dev));
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_rcm_keys(const int32_t *cand_dev, int64_t ncand, int64_t nrows, int32_t *parent_dev, const int32_t *rank_dev,
                             int64_t *keys_dev, void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_keys")) return st;
    if (ncand < 0 || ncand > nrows) return set_error(HPCLA_ERR_INVALID, "rcm_keys: needs 0 <= ncand <= nrows");
    if (ncand == 0) return HPCLA_OK;
    if (!cand_dev || !parent_dev || !rank_dev || !keys_dev) return set_error(HPCLA_ERR_INVALID, "rcm_keys: null array");
    rcm_keys_kernel<<<rcm_grid(ncand), RCM_THREADS, 0, as_stream(stream)>>>(cand_dev, ncand, nrows, parent_dev, rank_dev, keys_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_rcm_number(const int64_t *keys_dev, int64_t ncand, int64_t nrows, const int32_t *by_degree_dev, int64_t cnt,
                               int32_t *order_dev, void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_number")) return st;
    if (ncand < 0 || cnt < 0 || cnt + ncand > nrows) return set_error(HPCLA_ERR_INVALID, "rcm_number: needs 0 <= cnt, cnt + ncand <= nrows");
    if (ncand == 0) return HPCLA_OK;
    if (!keys_dev || !by_degree_dev || !order_dev) return set_error(HPCLA_ERR_INVALID, "rcm_number: null array");
    rcm_number_kernel<<<rcm_grid(ncand), RCM_THREADS, 0, as_stream(stream)>>>(keys_dev, ncand, nrows, by_degree_dev, cnt, order_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_rcm_finish(const int32_t *order_dev, int64_t nrows, int64_t row_start, int64_t *p_dev, int32_t *inv_dev,
                               void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_finish")) return st;
    if (nrows == 0) return HPCLA_OK;
    if (!order_dev || !p_dev || !inv_dev) return set_error(HPCLA_ERR_INVALID, "rcm_finish: null array");
    rcm_finish_kernel<<<rcm_grid(nrows), RCM_THREADS, 0, as_stream(stream)>>>(order_dev, nrows, row_start, p_dev, inv_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_rcm_graph_bandwidth(const int64_t *g_rowptr_dev, const int32_t *g_cols_dev, int64_t nrows, const int32_t *inv_dev,
                                        int64_t *out_dev, void *stream)
{
    if (int st = rcm_check_rows(nrows, "rcm_graph_bandwidth")) return st;
    if (!out_dev) return set_error(HPCLA_ERR_INVALID, "rcm_graph_bandwidth: null result");
    hipStream_t s = as_stream(stream);
    HPCLA_CHECK_HIP(hipMemsetAsync(out_dev, 0, sizeof(int64_t), s));
    if (nrows == 0) return HPCLA_OK;
    if (!g_rowptr_dev) return set_error(HPCLA_ERR_INVALID, "rcm_graph_bandwidth: null array");
    rcm_graph_bandwidth_kernel<<<rcm_grid(nrows), RCM_THREADS, 0, s>>>(g_rowptr_dev, g_cols_dev, nrows, inv_dev,
                                                                      reinterpret_cast<unsigned long long *>(out_dev));
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_bandwidth_i32(const int32_t *rowptr, const int32_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                                  int64_t row_start, int index_base, int64_t *out_dev, void *stream)
{
    return rcm_matrix_bandwidth_impl<int32_t>(rowptr, colval, col_indices_dev, nrows, row_start, index_base, out_dev, stream);
}

HPCLA_API int hpcla_bandwidth_i64(const int64_t *rowptr, const int64_t *colval, const int64_t *col_indices_dev, int64_t nrows,
                                  int64_t row_start, int index_base, int64_t *out_dev, void *stream)
{
    return rcm_matrix_bandwidth_impl<int64_t>(rowptr, colval, col_indices_dev, nrows, row_start, index_base, out_dev, stream);
}
