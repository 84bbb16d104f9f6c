// gram.hip -- C = transpose(X) * Y of two tall row-partitioned dense blocks (the small inner-product matrix of block
// methods: block CG, LOBPCG, Rayleigh-Ritz, CholQR).
//
// Reference: Base.:*(At::TransposedHPCMatrix, Bmat::HPCMatrix) (src/dense.jl:1286-1310) builds the product one column
// at a time -- k calls of transpose(A) * b_col, each a column copy, a full read of X and a host all-reduce.  Here ONE
// pass reads X and Y once and forms every C[i][j] = sum_r X[r][i] * Y[r][j] of the local rows, then one all-reduce of
// the m x k doubles (allreduce_on: RCCL, or the peer window).
//
// Stage 1: v_mfma_f64_16x16x4_f64.  A wavefront multiplies a 16-column tile of X (the A operand: lane l holds
// X[row(l>>4)][16 ti + (l&15)]) by a 16-column tile of Y (B operand: Y[row(l>>4)][16 tj + (l&15)]) over 4 rows per
// instruction -- the operands load straight from global memory in the MFMA's own lane map, whatever the layout (a lane
// reads one element; row-major consecutive lanes read consecutive columns).  A workgroup (4 waves) owns a fixed chunk
// of rows and a panel of up to (16 TN) x (16 TN) outputs; each wave takes 8 of every 32 rows (two MFMA k-groups), U
// such steps of loads in flight.  C/D lane map of the f64 form: col = lane & 15, row = (lane >> 4) + 4 * reg.
// The 4 waves' tiles are added in wave order through LDS into partial[chunk][m][k].
// Stage 2: each output entry sums the chunks in a fixed tree (64 phases, each ascending, then the phases ascending).
// The chunking depends on (nrows, m, k) only, so the same inputs give the same bits on every call.
//
// Symmetric case (X and Y the same block): a tile is loaded once and used as both operands, only tiles with ti <= tj
// are multiplied, and stage 2 sums the entries with i <= j and writes each to both C[i][j] and C[j][i]; after a
// multi-rank all-reduce the upper triangle is mirrored again, so C is exactly symmetric.
//
// Float32: every element is widened to double on load; products (exact) and sums are double, and C is double -- the
// caller rounds to float once, after the all-reduce.
#include "common.h"

namespace hpcla {

int allreduce_on(hpcla_comm_t *comm, double *buf, int64_t count, int op, void *stream);  // comm.hip

typedef double gram_d4 __attribute__((ext_vector_type(4)));

constexpr int GRAM_THREADS = 256;            // 4 waves
constexpr int GRAM_STEP_ROWS = 32;           // rows per workgroup step: 8 per wave = 2 MFMA k-groups of 4
constexpr int64_t GRAM_MIN_CHUNK = 256;      // rows per chunk at least
constexpr int GRAM2_THREADS = 1024;
constexpr int GRAM2_CT = 16;                 // output entries per stage-2 workgroup (one 128-byte line of a partial)

__device__ __forceinline__ gram_d4 mfma_f64(double a, double b, gram_d4 c)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// Element (r, c) of a block is p[r * rs + c * cs]: row-major (rs, cs) = (ld, 1), column-major (1, ld).
template <typename T, int TN, int U>
__global__ __launch_bounds__(GRAM_THREADS) void gram_stage1(const T *__restrict__ X, int64_t xrs, int64_t xcs,
                                                             const T *__restrict__ Y, int64_t yrs, int64_t ycs,
                                                             int64_t nrows, int64_t m, int64_t k, int64_t rows_per_chunk,
                                                             int64_t panels_k, int sym, double *__restrict__ partial)
{
    __shared__ double red[GRAM_THREADS / 64][256];
    const int tid = threadIdx.x;
    const int w = tid >> 6, lane = tid & 63;
    const int q = lane >> 4, c = lane & 15;
    const int64_t chunk = blockIdx.x;
    const int64_t pi = (int64_t)blockIdx.y / panels_k, pj = (int64_t)blockIdx.y % panels_k;
    if (sym && pi > pj) return;                          // the mirror of a panel already computed
    const bool diag = sym && pi == pj;                   // one operand serves both sides
    const int64_t i0 = pi * 16 * TN, j0 = pj * 16 * TN;
    const int64_t r0 = chunk * rows_per_chunk;
    const int64_t r1 = min(nrows, r0 + rows_per_chunk);

    const T *px[TN];
    const T *py[TN];
    bool okx[TN], oky[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const int64_t ci = i0 + 16 * t + c, cj = j0 + 16 * t + c;
        okx[t] = ci < m;
        oky[t] = cj < k;
        px[t] = X + (okx[t] ? ci * xcs : 0);
        py[t] = Y + (oky[t] ? cj * ycs : 0);
    }
    gram_d4 acc[TN][TN];
#pragma unroll
    for (int ti = 0; ti < TN; ++ti)
#pragma unroll
        for (int tj = 0; tj < TN; ++tj) acc[ti][tj] = (gram_d4)(0.0);

    // one pass of U workgroup steps; CHECK = rows may run past r1 (the chunk's last pass)
    auto pass = [&](int64_t base, bool check) __attribute__((always_inline)) {
        double a[U][2][TN], b[U][2][TN];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int64_t r = base + (int64_t)u * GRAM_STEP_ROWS + 8 * w + 2 * q + h;
                const bool rok = !check || r < r1;
                const int64_t ox = r * xrs, oy = r * yrs;
#pragma unroll
                for (int t = 0; t < TN; ++t) a[u][h][t] = (rok && okx[t]) ? (double)px[t][ox] : 0.0;
                if (!diag) {
#pragma unroll
                    for (int t = 0; t < TN; ++t) b[u][h][t] = (rok && oky[t]) ? (double)py[t][oy] : 0.0;
                }
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int ti = 0; ti < TN; ++ti)
#pragma unroll
                    for (int tj = 0; tj < TN; ++tj) {
                        if (diag && ti > tj) continue;
                        acc[ti][tj] = mfma_f64(a[u][h][ti], diag ? a[u][h][tj] : b[u][h][tj], acc[ti][tj]);
                    }
    };
    const int64_t pass_rows = (int64_t)U * GRAM_STEP_ROWS;
    int64_t base = r0;
    for (; base + pass_rows <= r1; base += pass_rows) pass(base, false);
    if (base < r1) pass(base, true);

    // the 4 waves' tiles, added in wave order
    double *out = partial + chunk * m * k;
#pragma unroll
    for (int ti = 0; ti < TN; ++ti)
#pragma unroll
        for (int tj = 0; tj < TN; ++tj) {
            if (diag && ti > tj) continue;
            if (i0 + 16 * ti >= m || j0 + 16 * tj >= k) continue;       // uniform: the tile lies outside C
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) red[w][(q + 4 * reg) * 16 + c] = acc[ti][tj][reg];
            __syncthreads();
            const int e = tid;                                          // 256 threads = the 16 x 16 tile
            const int64_t gi = i0 + 16 * ti + (e >> 4), gj = j0 + 16 * tj + (e & 15);
            if (gi < m && gj < k) out[gi * k + gj] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
            __syncthreads();
        }
}

// Stage 2: C[i][j] = sum over chunks of partial[chunk][i][j], 64 phases of ascending chunks, phases ascending.
__global__ __launch_bounds__(GRAM2_THREADS) void gram_stage2(const double *__restrict__ partial, int64_t nchunks,
                                                             int64_t m, int64_t k, int sym, double *__restrict__ C)
{
    __shared__ double red[GRAM2_THREADS];
    const int tid = threadIdx.x;
    const int cc = tid % GRAM2_CT, ph = tid / GRAM2_CT;
    constexpr int nph = GRAM2_THREADS / GRAM2_CT;
    const int64_t mk = m * k;
    const int64_t e = (int64_t)blockIdx.x * GRAM2_CT + cc;
    const int64_t i = e / (k > 0 ? k : 1), j = e - i * k;
    const bool live = e < mk && !(sym && i > j);
    double s = 0.0;
    if (live) {
        int64_t ch = ph;
        for (; ch + 7 * nph < nchunks; ch += 8 * (int64_t)nph) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(ch + (int64_t)u * nph) * mk + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; ch < nchunks; ch += nph) s += partial[ch * mk + e];
    }
    red[tid] = s;
    __syncthreads();
    if (ph == 0 && live) {
        double t = red[cc];
        for (int p = 1; p < nph; ++p) t += red[p * GRAM2_CT + cc];
        C[e] = t;
        if (sym && i != j) C[j * k + i] = t;
    }
}

// C[j][i] = C[i][j] for i < j (after an all-reduce, whose element order may differ between mirrored positions)
__global__ __launch_bounds__(256) void gram_mirror(double *__restrict__ C, int64_t m)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m * m) return;
    const int64_t i = e / m, j = e - i * m;
    if (i > j) C[e] = C[j * m + i];
}

static int gram_tn(int64_t m, int64_t k)
{
    const int64_t w = m > k ? m : k;
    return w <= 16 ? 1 : (w <= 32 ? 2 : 4);
}

// chunks wanted: ~2048 stage-1 workgroups over all panels (8 per CU), and at most 4 Mi partial doubles (32 MiB) to
// keep stage 2 small against stage 1
static int64_t gram_want_chunks(int64_t m, int64_t k)
{
    const int64_t pw = 16 * (int64_t)gram_tn(m, k);
    const int64_t panels = ((m + pw - 1) / pw) * ((k + pw - 1) / pw);
    int64_t want = (2048 + panels - 1) / panels;
    const int64_t cap = ((int64_t)4 << 20) / (m * k);
    if (want > cap) want = cap;
    return want < 1 ? 1 : want;
}

static int64_t gram_rows_per_chunk(int64_t nrows, int64_t m, int64_t k)
{
    const int64_t want = gram_want_chunks(m, k);
    int64_t rpc = (nrows + want - 1) / want;
    rpc = (rpc + GRAM_MIN_CHUNK - 1) / GRAM_MIN_CHUNK * GRAM_MIN_CHUNK;
    return rpc < GRAM_MIN_CHUNK ? GRAM_MIN_CHUNK : rpc;
}

// an upper bound of ceil(nrows / rows_per_chunk) that is monotone in nrows: min(ceil(nrows / 256), want)
static int64_t gram_max_chunks(int64_t nrows, int64_t m, int64_t k)
{
    const int64_t by_rows = (nrows + GRAM_MIN_CHUNK - 1) / GRAM_MIN_CHUNK;
    const int64_t want = gram_want_chunks(m, k);
    return by_rows < want ? by_rows : want;
}

template <typename T>
static int gram_impl(const char *who, hpcla_comm_t *comm, const T *X, int64_t ldx, int x_layout, const T *Y, int64_t ldy,
                     int y_layout, int64_t nrows, int64_t m, int64_t k, double *C, void *work, void *stream)
{
    if (nrows < 0 || m < 0 || k < 0) return set_error(HPCLA_ERR_INVALID, "%s: negative size", who);
    if ((x_layout != HPCLA_LAYOUT_ROW && x_layout != HPCLA_LAYOUT_COL) ||
        (y_layout != HPCLA_LAYOUT_ROW && y_layout != HPCLA_LAYOUT_COL))
        return set_error(HPCLA_ERR_INVALID, "%s: layout must be HPCLA_LAYOUT_ROW or HPCLA_LAYOUT_COL", who);
    if (ldx < (x_layout == HPCLA_LAYOUT_ROW ? m : nrows) || ldy < (y_layout == HPCLA_LAYOUT_ROW ? k : nrows))
        return set_error(HPCLA_ERR_INVALID, "%s: leading dimension smaller than the block", who);
    if (m == 0 || k == 0) return HPCLA_OK;
    if (m > 0x7fffffffLL / k) return set_error(HPCLA_ERR_UNSUPPORTED, "%s: m * k too large", who);
    if (!C) return set_error(HPCLA_ERR_INVALID, "%s: null C", who);
    hipStream_t s = as_stream(stream);
    // the symmetric case needs a real pointer: a rank without rows passes NULL for both blocks unless the product is
    // X'X, and then the same non-NULL pointer (it decides whether C is mirrored after the all-reduce, as on the others)
    const bool sym = X == Y && X != nullptr && x_layout == y_layout && ldx == ldy && m == k;
    if (nrows == 0) {                                    // no local rows: the partial is zero, the rank still reduces
        HPCLA_CHECK_HIP(hipMemsetAsync(C, 0, (size_t)(m * k) * sizeof(double), s));
    } else {
        if (!X || !Y || !work) return set_error(HPCLA_ERR_INVALID, "%s: null X / Y / work", who);
        if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Y)) % sizeof(T))
            return set_error(HPCLA_ERR_INVALID, "%s: X and Y must be aligned to their element size", who);
        const int tn = gram_tn(m, k);
        const int64_t pw = 16 * (int64_t)tn;
        const int64_t pm = (m + pw - 1) / pw, pk = (k + pw - 1) / pw;
        const int64_t rpc = gram_rows_per_chunk(nrows, m, k);
        const int64_t nchunks = (nrows + rpc - 1) / rpc;
        if (nchunks > gram_max_chunks(nrows, m, k)) return set_error(HPCLA_ERR_INVALID, "%s: chunk count", who);
        if (pm * pk > 65535) return set_error(HPCLA_ERR_UNSUPPORTED, "%s: more than 65535 output panels", who);
        const int64_t xrs = x_layout == HPCLA_LAYOUT_ROW ? ldx : 1, xcs = x_layout == HPCLA_LAYOUT_ROW ? 1 : ldx;
        const int64_t yrs = y_layout == HPCLA_LAYOUT_ROW ? ldy : 1, ycs = y_layout == HPCLA_LAYOUT_ROW ? 1 : ldy;
        double *partial = static_cast<double *>(work);
        const dim3 grid((uint32_t)nchunks, (uint32_t)(pm * pk));
        if (tn == 1)
            gram_stage1<T, 1, 4><<<grid, GRAM_THREADS, 0, s>>>(X, xrs, xcs, Y, yrs, ycs, nrows, m, k, rpc, pk, sym, partial);
        else if (tn == 2)
            gram_stage1<T, 2, 4><<<grid, GRAM_THREADS, 0, s>>>(X, xrs, xcs, Y, yrs, ycs, nrows, m, k, rpc, pk, sym, partial);
        else
            gram_stage1<T, 4, 2><<<grid, GRAM_THREADS, 0, s>>>(X, xrs, xcs, Y, yrs, ycs, nrows, m, k, rpc, pk, sym, partial);
        HPCLA_CHECK_LAUNCH();
        gram_stage2<<<(uint32_t)((m * k + GRAM2_CT - 1) / GRAM2_CT), GRAM2_THREADS, 0, s>>>(partial, nchunks, m, k,
                                                                                            sym, C);
        HPCLA_CHECK_LAUNCH();
    }
    if (comm) {
        const int st = allreduce_on(comm, C, m * k, 0, stream);
        if (st != HPCLA_OK) return st;
        if (sym) {
            gram_mirror<<<(uint32_t)((m * m + 255) / 256), 256, 0, s>>>(C, m);
            HPCLA_CHECK_LAUNCH();
        }
    }
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_gram_work_bytes(int64_t nrows, int64_t m, int64_t k)
{
    if (nrows <= 0 || m <= 0 || k <= 0 || m > 0x7fffffffLL / k) return 8;
    return gram_max_chunks(nrows, m, k) * m * k * (int64_t)sizeof(double);
}

HPCLA_API int hpcla_gram_f64(hpcla_comm_t *comm, const double *X, int64_t ldx, int x_layout, const double *Y,
                             int64_t ldy, int y_layout, int64_t nrows, int64_t m, int64_t k, double *C, void *work,
                             void *stream)
{
    return gram_impl<double>("gram_f64", comm, X, ldx, x_layout, Y, ldy, y_layout, nrows, m, k, C, work, stream);
}

HPCLA_API int hpcla_gram_f32(hpcla_comm_t *comm, const float *X, int64_t ldx, int x_layout, const float *Y,
                             int64_t ldy, int y_layout, int64_t nrows, int64_t m, int64_t k, double *C, void *work,
                             void *stream)
{
    return gram_impl<float>("gram_f32", comm, X, ldx, x_layout, Y, ldy, y_layout, nrows, m, k, C, work, stream);
}
