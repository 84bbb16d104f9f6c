// lobpcg.hip -- the tall-block kernels of the block eigensolver (hp.lobpcg): the residual block with its column norms (one
// kernel for A x = lambda x, one for the pencil A x = lambda B x), and the in-place combine [X | P] <- S C of the Rayleigh-Ritz
// step.
//
// Every block is row-major: row r of a block is k doubles at a pitch (in doubles) of its own, so the blocks may be column
// ranges of one wider buffer -- the solver keeps [X W P | AX AW AP] in one (n, 6k) buffer, and [X W P | AX AW AP | BX BW BP]
// in one (n, 9k) buffer with a B.  1 <= k <= 16.
//
// RESIDUAL.  t = theta[j] * X[r,j];  d = AX[r,j] - t;  W[r,j] = minv[r] * d (or d): three separately rounded operations
// (-ffp-contract=off).  A lane owns a (row, column pair): with even pitches and 16-byte aligned bases a pair is one 16-byte
// access (the last column of an odd k is an 8-byte access), otherwise the same lanes make 8-byte accesses.  With a pitch equal
// to k consecutive lanes touch consecutive addresses.  A lane keeps its column pair for all its rows, so the sums of squares
// of d (the residual before minv) are per-lane sums per column.  Stage 1: a workgroup owns LOB_CHUNK_ROWS-row multiples (the chunk length is a function
// of (n, k) only), lane (row slot s, pair c) walks rows s, s + RP, ... of the chunk; the slots are added through LDS in
// LOB_PHASES phases (slot g, g + 16, ... ascending, then the phases ascending) into partial[chunk][k].  Stage 2: one workgroup
// adds the chunks the same way (LOB_PHASES phases of ascending chunks, then the phases ascending).  Every order is fixed by
// (n, k): the same inputs give the same bits on every call.  Then one all-reduce of the k sums (allreduce_on, comm.hip).
// Bytes per row: read 8 (2k + 1 with minv), write 8k (16k with the second copy of W, which the SpMM reads on its own pitch).
//
// RESIDUAL OF THE PENCIL (lobpcg_residual_gen_kernel).  t = theta[j] * BX[r,j];  d = AX[r,j] - t;  w = minv[r] * d (or d);
// W[r,j] = w;  W2[r,j] = w (if given);  BW[r,j] = bdiag[r] * w (if B is a diagonal: B W needs no product then): every operation
// separately rounded.  Three sums per column, sum d^2, sum AX^2 and sum BX^2: the stop rule of the pencil,
// ||A x - theta B x|| <= tol (||A x|| + |theta| ||B x||), takes all four norms from this one pass.  Mapping, chunking and both
// fixed summation orders are those of the kernel above with three accumulators per column: a lane's rows ascending, the slots
// through LDS in LOB_PHASES phases into partial[chunk][3][k], one workgroup over the chunks (a lane adds the three groups side by side, so
// the loads of a chunk are one chain and not three), then ONE all-reduce of 48 doubles (group q at sums + 16 q; the entries j >= k of a group are not written by the
// kernels).  LDS 18 KiB per workgroup of four waves would allow eight workgroups per CU; the six accumulators and the two
// unrolled rows in flight take 80 VGPRs (78 on the 8-byte path), no spill, so the registers bound it at six waves per SIMD,
// 24 per CU, which a streaming kernel of this kind does not feel (the kernel above: 52 VGPRs, eight waves).
// Bytes per row: read 16k (+8 with minv, +8 with bdiag), write 8k per output block (W, W2, BW).
//
// COMBINE.  S = [X W P] holds k + c_rest input columns (c_rest = 0: X alone; k: [X W]; 2k: [X W P]); C is (k + c_rest) x k,
// row i at C + 16 i.  Per row and output column j
//     px = 0;  px = px + S[r,i] * C[i,j]  for i = 0 .. k-1 ascending
//     pp = 0;  pp = pp + S[r,i] * C[i,j]  for i = k .. k + c_rest - 1 ascending
//     X'[r,j] = px + pp;   P'[r,j] = pp  (no P' with c_rest = 0)
// products and sums separately rounded (plain multiplies and adds, no MFMA).  The same for AS = [AX AW AP] (the odd workgroups).
// Mapping: ROWS ARE STAGED THROUGH LDS (eigsh_rotate's one-lane-one-row mapping does not coalesce in row-major at a 384-byte
// pitch).  A workgroup of 256 lanes owns a tile of 256 / (KT / 4) rows, KT = 4, 8 or 16 >= k: 256, 128 or 64.  (a) All lanes load
// the tile's k + c_rest columns with the coalesced (row, column pair) walk of the residual kernel into LDS, at an odd row
// stride so that different rows start in different banks, and C as it was uploaded (it is the same for every row).
// (b) Barrier.  KT / 4 adjacent lanes share a row and each owns 4 output columns: a lane reads its row from LDS one value at a
// time (the lanes of a row read the same address: a broadcast) with the 4 coefficients of its columns and updates its 8
// accumulators; columns j >= k of the 16-wide rows of C are read and their sums never stored.  After a barrier (the lanes that
// share the row have read it) the lane writes its part of X' and P' over the LDS row.  (c) Barrier, then the same coalesced
// walk stores the X' and P' columns.  At most 32 KiB of LDS per workgroup: five workgroups, twenty waves per CU.
// In place: a row is read and written by exactly one workgroup, and every global load of the tile is complete -- its value
// sits in LDS -- before the first barrier, while every global store comes after the last.  The W columns are never stored.
// Bytes per row: read 16 (k + c_rest), write 32k (16k with c_rest = 0).
// No loop in this file waits on memory another workgroup writes.
#include "common.h"

namespace hpcla {

int allreduce_on(hpcla_comm_t *comm, double *buf, int64_t count, int op, void *stream);  // comm.hip

constexpr int LOB_MAX_K = 16;
constexpr int LOB_THREADS = 256;
constexpr int LOB_PHASES = 16;                 // phases of both fixed-order sums
constexpr int64_t LOB_CHUNK_ROWS = 1024;       // a stage-1 workgroup owns a multiple of this many rows
constexpr int64_t LOB_MAX_CHUNKS = 2048;       // stage-1 workgroups at most
constexpr int LOB_JPL = 4;                     // output columns of a combine lane
constexpr int LOB_C_DOUBLES = 3 * LOB_MAX_K * LOB_MAX_K;   // C in LDS: at most 48 rows of 16

static int64_t lob_rows_per_chunk(int64_t n)
{
    int64_t rpc = (n + LOB_MAX_CHUNKS - 1) / LOB_MAX_CHUNKS;
    rpc = (rpc + LOB_CHUNK_ROWS - 1) / LOB_CHUNK_ROWS * LOB_CHUNK_ROWS;
    return rpc < LOB_CHUNK_ROWS ? LOB_CHUNK_ROWS : rpc;
}

// ---- residual ---------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(LOB_THREADS) void lobpcg_residual_kernel(const double *__restrict__ X, int64_t ldx,
                                                                      const double *__restrict__ AX, int64_t ldax,
                                                                      const double *__restrict__ theta,
                                                                      const double *__restrict__ minv, double *__restrict__ W,
                                                                      int64_t ldw, double *__restrict__ W2, int64_t ldw2,
                                                                      int64_t n, int k, int64_t rows_per_chunk,
                                                                      double *__restrict__ partial)
{
    __shared__ double red[LOB_THREADS][2];
    __shared__ double ph[LOB_PHASES][LOB_MAX_K];
    const int tid = threadIdx.x;
    const int kp = (k + 1) >> 1;                     // column pairs of a row
    const int RP = LOB_THREADS / kp;                 // rows of one pass of the workgroup
    const int slot = tid / kp, c = tid - slot * kp;
    const int j0 = 2 * c;
    const bool two = j0 + 1 < k;                     // the pair's second column exists
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk;
    const int64_t r1 = min(n, r0 + rows_per_chunk);
    double a0 = 0.0, a1 = 0.0;
    if (slot < RP) {
        const double th0 = theta[j0], th1 = two ? theta[j0 + 1] : 0.0;
#pragma unroll 2
        for (int64_t r = r0 + slot; r < r1; r += RP) {
            double x0, x1 = 0.0, y0, y1 = 0.0;
            if (VEC && two) {
                const double2 xv = *reinterpret_cast<const double2 *>(X + r * ldx + j0);
                const double2 yv = *reinterpret_cast<const double2 *>(AX + r * ldax + j0);
                x0 = xv.x, x1 = xv.y, y0 = yv.x, y1 = yv.y;
            } else {
                x0 = X[r * ldx + j0], y0 = AX[r * ldax + j0];
                if (two) x1 = X[r * ldx + j0 + 1], y1 = AX[r * ldax + j0 + 1];
            }
            const double t0 = th0 * x0, t1 = th1 * x1;
            double w0 = y0 - t0, w1 = y1 - t1;
            a0 = a0 + w0 * w0;                       // the norms are those of R = AX - X diag(theta), not of M .* R
            if (two) a1 = a1 + w1 * w1;
            if (minv) {
                const double mi = minv[r];
                w0 = mi * w0, w1 = mi * w1;
            }
            if (VEC && two) {
                *reinterpret_cast<double2 *>(W + r * ldw + j0) = make_double2(w0, w1);
                if (W2) *reinterpret_cast<double2 *>(W2 + r * ldw2 + j0) = make_double2(w0, w1);
            } else {
                W[r * ldw + j0] = w0;
                if (two) W[r * ldw + j0 + 1] = w1;
                if (W2) {
                    W2[r * ldw2 + j0] = w0;
                    if (two) W2[r * ldw2 + j0 + 1] = w1;
                }
            }
        }
    }
    red[tid][0] = a0;
    red[tid][1] = a1;
    __syncthreads();
    if (tid < LOB_PHASES * k) {                      // phase g of column j: slots g, g + 16, ... ascending
        const int g = tid / k, j = tid - g * k;
        double s = 0.0;
        for (int sl = g; sl < RP; sl += LOB_PHASES) s = s + red[sl * kp + (j >> 1)][j & 1];
        ph[g][j] = s;
    }
    __syncthreads();
    if (tid < k) {
        double s = ph[0][tid];
        for (int g = 1; g < LOB_PHASES; ++g) s = s + ph[g][tid];
        partial[(int64_t)blockIdx.x * k + tid] = s;
    }
}

// out[j] = sum over chunks of partial[chunk][j]: LOB_PHASES phases of ascending chunks, then the phases ascending
__global__ __launch_bounds__(LOB_THREADS) void lobpcg_residual_stage2(const double *__restrict__ partial, int64_t nchunks, int k,
                                                                      double *__restrict__ out)
{
    __shared__ double ph[LOB_PHASES][LOB_MAX_K];
    const int tid = threadIdx.x;
    if (tid < LOB_PHASES * k) {
        const int g = tid / k, j = tid - g * k;
        double s = 0.0;
        for (int64_t ch = g; ch < nchunks; ch += LOB_PHASES) s = s + partial[ch * k + j];
        ph[g][j] = s;
    }
    __syncthreads();
    if (tid < k) {
        double s = ph[0][tid];
        for (int g = 1; g < LOB_PHASES; ++g) s = s + ph[g][tid];
        out[tid] = s;
    }
}

// ---- residual of the pencil (A, B) ------------------------------------------------------------------------------------------
constexpr int LOB_GEN_SUMS = 3;                // sum d^2, sum AX^2, sum BX^2 per column

template <bool VEC>
__global__ __launch_bounds__(LOB_THREADS) void lobpcg_residual_gen_kernel(const double *__restrict__ AX, int64_t ldax,
                                                                          const double *__restrict__ BX, int64_t ldbx,
                                                                          const double *__restrict__ theta,
                                                                          const double *__restrict__ minv,
                                                                          const double *__restrict__ bdiag, double *__restrict__ W,
                                                                          int64_t ldw, double *__restrict__ W2, int64_t ldw2,
                                                                          double *__restrict__ BW, int64_t ldbw, int64_t n, int k,
                                                                          int64_t rows_per_chunk, double *__restrict__ partial)
{
    __shared__ double red[LOB_GEN_SUMS][LOB_THREADS][2];
    __shared__ double ph[LOB_GEN_SUMS][LOB_PHASES][LOB_MAX_K];
    const int tid = threadIdx.x;
    const int kp = (k + 1) >> 1;                     // column pairs of a row
    const int RP = LOB_THREADS / kp;                 // rows of one pass of the workgroup
    const int slot = tid / kp, c = tid - slot * kp;
    const int j0 = 2 * c;
    const bool two = j0 + 1 < k;                     // the pair's second column exists
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk;
    const int64_t r1 = min(n, r0 + rows_per_chunk);
    double d0 = 0.0, d1 = 0.0, a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    if (slot < RP) {
        const double th0 = theta[j0], th1 = two ? theta[j0 + 1] : 0.0;
#pragma unroll 2
        for (int64_t r = r0 + slot; r < r1; r += RP) {
            double x0, x1 = 0.0, y0, y1 = 0.0;       // x: B X, y: A X
            if (VEC && two) {
                const double2 xv = *reinterpret_cast<const double2 *>(BX + r * ldbx + j0);
                const double2 yv = *reinterpret_cast<const double2 *>(AX + r * ldax + j0);
                x0 = xv.x, x1 = xv.y, y0 = yv.x, y1 = yv.y;
            } else {
                x0 = BX[r * ldbx + j0], y0 = AX[r * ldax + j0];
                if (two) x1 = BX[r * ldbx + j0 + 1], y1 = AX[r * ldax + j0 + 1];
            }
            const double t0 = th0 * x0, t1 = th1 * x1;
            double w0 = y0 - t0, w1 = y1 - t1;
            d0 = d0 + w0 * w0;                       // the norms are those of A X - B X diag(theta), not of M .* R
            a0 = a0 + y0 * y0;
            b0 = b0 + x0 * x0;
            if (two) {
                d1 = d1 + w1 * w1;
                a1 = a1 + y1 * y1;
                b1 = b1 + x1 * x1;
            }
            if (minv) {
                const double mi = minv[r];
                w0 = mi * w0, w1 = mi * w1;
            }
            if (VEC && two) {
                *reinterpret_cast<double2 *>(W + r * ldw + j0) = make_double2(w0, w1);
                if (W2) *reinterpret_cast<double2 *>(W2 + r * ldw2 + j0) = make_double2(w0, w1);
            } else {
                W[r * ldw + j0] = w0;
                if (two) W[r * ldw + j0 + 1] = w1;
                if (W2) {
                    W2[r * ldw2 + j0] = w0;
                    if (two) W2[r * ldw2 + j0 + 1] = w1;
                }
            }
            if (bdiag) {                             // a diagonal B: B W is a row scaling of what was just stored
                const double bd = bdiag[r];
                const double v0 = bd * w0, v1 = bd * w1;
                if (VEC && two) {
                    *reinterpret_cast<double2 *>(BW + r * ldbw + j0) = make_double2(v0, v1);
                } else {
                    BW[r * ldbw + j0] = v0;
                    if (two) BW[r * ldbw + j0 + 1] = v1;
                }
            }
        }
    }
    red[0][tid][0] = d0, red[0][tid][1] = d1;
    red[1][tid][0] = a0, red[1][tid][1] = a1;
    red[2][tid][0] = b0, red[2][tid][1] = b1;
    __syncthreads();
    if (tid < LOB_PHASES * k) {                      // phase g of column j: slots g, g + 16, ... ascending, per group
        const int g = tid / k, j = tid - g * k;
        for (int q = 0; q < LOB_GEN_SUMS; ++q) {
            double s = 0.0;
            for (int sl = g; sl < RP; sl += LOB_PHASES) s = s + red[q][sl * kp + (j >> 1)][j & 1];
            ph[q][g][j] = s;
        }
    }
    __syncthreads();
    if (tid < LOB_GEN_SUMS * k) {
        const int q = tid / k, j = tid - q * k;
        double s = ph[q][0][j];
        for (int g = 1; g < LOB_PHASES; ++g) s = s + ph[q][g][j];
        partial[((int64_t)blockIdx.x * LOB_GEN_SUMS + q) * k + j] = s;
    }
}

// out[16 q + j] = sum over chunks of partial[chunk][q][j]: LOB_PHASES phases of ascending chunks, then the phases ascending
__global__ __launch_bounds__(LOB_THREADS) void lobpcg_residual_gen_stage2(const double *__restrict__ partial, int64_t nchunks,
                                                                          int k, double *__restrict__ out)
{
    __shared__ double ph[LOB_GEN_SUMS][LOB_PHASES][LOB_MAX_K];
    const int tid = threadIdx.x;
    if (tid < LOB_PHASES * k) {                      // the three groups side by side: one chain of loads, not three in a row
        const int g = tid / k, j = tid - g * k;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int64_t ch = g; ch < nchunks; ch += LOB_PHASES) {
            const double *p = partial + ch * LOB_GEN_SUMS * k + j;
            s0 = s0 + p[0];
            s1 = s1 + p[k];
            s2 = s2 + p[2 * k];
        }
        ph[0][g][j] = s0, ph[1][g][j] = s1, ph[2][g][j] = s2;
    }
    __syncthreads();
    if (tid < LOB_GEN_SUMS * k) {
        const int q = tid / k, j = tid - q * k;
        double s = ph[q][0][j];
        for (int g = 1; g < LOB_PHASES; ++g) s = s + ph[q][g][j];
        out[q * LOB_MAX_K + j] = s;
    }
}

// ---- combine ----------------------------------------------------------------------------------------------------------------
// columns [c0, c0 + nc) of the tile's ROWS rows between global memory (pitch ld) and LDS (row stride ldl): the workgroup's lanes
// walk (row, column pair) items in row-major order, LOB_THREADS items at a time.  TO_LDS: rows past n load as zero;  else rows
// past n are not stored
template <bool VEC, bool TO_LDS, int ROWS>
__device__ __forceinline__ void lob_tile_copy(double *G, int64_t ld, double *lds, int ldl, int c0, int nc, int64_t row0, int64_t n,
                                              int tid)
{
    const int hp = VEC ? nc >> 1 : nc;               // items of a row (VEC: nc is even)
    const int dr = LOB_THREADS / hp, dc = LOB_THREADS - dr * hp;
    int row = tid / hp, cp = tid - row * hp;
    while (row < ROWS) {
        const int64_t r = row0 + row;
        const int col = c0 + (VEC ? 2 * cp : cp);
        if (TO_LDS) {
            if (VEC) {
                double2 v = make_double2(0.0, 0.0);
                if (r < n) v = *reinterpret_cast<const double2 *>(G + r * ld + col);
                lds[row * ldl + col] = v.x;
                lds[row * ldl + col + 1] = v.y;
            } else {
                lds[row * ldl + col] = r < n ? G[r * ld + col] : 0.0;
            }
        } else if (r < n) {
            if (VEC) *reinterpret_cast<double2 *>(G + r * ld + col) = make_double2(lds[row * ldl + col], lds[row * ldl + col + 1]);
            else G[r * ld + col] = lds[row * ldl + col];
        }
        row += dr;
        cp += dc;
        if (cp >= hp) cp -= hp, ++row;
    }
}

// KT = 4, 8 or 16 >= k: KT / 4 lanes share a row, each owns LOB_JPL = 4 output columns
template <int KT, bool VEC>
__global__ __launch_bounds__(LOB_THREADS) void lobpcg_combine_kernel(double *S, int64_t lds_, double *AS, int64_t ldas,
                                                                     const double *__restrict__ C, int k, int c_rest, int64_t n)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int LPR = KT / LOB_JPL, ROWS = LOB_THREADS / LPR;
    double *Cl = smem;                               // C as uploaded: (k + c_rest) rows of 16
    double *tile = smem + LOB_C_DOUBLES;             // ROWS rows at the stride ldl
    const int tid = threadIdx.x;
    const int c_in = k + c_rest;
    const int ldl = (c_rest ? 3 * k : k) | 1;        // the row holds P' too; odd stride: the rows start in different banks
    // workgroups 2t and 2t + 1 take tile t of S and of AS: where both are column ranges of one buffer they share its lines
    const int64_t t = AS ? blockIdx.x >> 1 : blockIdx.x;
    const bool second = AS && (blockIdx.x & 1);
    double *G = second ? AS : S;                     // no __restrict__: the stores alias the loads on purpose
    const int64_t ld = second ? ldas : lds_;
    const int64_t row0 = t * ROWS;

    for (int e = tid; e < c_in * LOB_MAX_K; e += LOB_THREADS) Cl[e] = C[e];
    lob_tile_copy<VEC, true, ROWS>(G, ld, tile, ldl, 0, c_in, row0, n, tid);
    __syncthreads();

    const int row = tid / LPR, j0 = LOB_JPL * (tid - row * LPR);
    double *mine = tile + row * ldl;
    const double *Cg = Cl + j0;
    double px[LOB_JPL], pp[LOB_JPL];
#pragma unroll
    for (int j = 0; j < LOB_JPL; ++j) px[j] = 0.0, pp[j] = 0.0;
#pragma unroll 4
    for (int i = 0; i < k; ++i) {
        const double s = mine[i];
#pragma unroll
        for (int j = 0; j < LOB_JPL; ++j) px[j] = px[j] + s * Cg[i * LOB_MAX_K + j];
    }
#pragma unroll 4
    for (int i = k; i < c_in; ++i) {
        const double s = mine[i];
#pragma unroll
        for (int j = 0; j < LOB_JPL; ++j) pp[j] = pp[j] + s * Cg[i * LOB_MAX_K + j];
    }
    __syncthreads();                                 // the lanes that share this row have read it
#pragma unroll
    for (int j = 0; j < LOB_JPL; ++j)
        if (j0 + j < k) {
            mine[j0 + j] = px[j] + pp[j];
            if (c_rest) mine[2 * k + j0 + j] = pp[j];
        }
    __syncthreads();

    lob_tile_copy<VEC, false, ROWS>(G, ld, tile, ldl, 0, k, row0, n, tid);
    if (c_rest) lob_tile_copy<VEC, false, ROWS>(G, ld, tile, ldl, 2 * k, k, row0, n, tid);
}

static bool lob_even_aligned(const void *p, int64_t ld) { return !p || (!(reinterpret_cast<uintptr_t>(p) & 15) && !(ld & 1)); }

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_lobpcg_chunk_rows(int64_t n) { return n > 0 ? lob_rows_per_chunk(n) : LOB_CHUNK_ROWS; }

HPCLA_API int64_t hpcla_lobpcg_work_bytes(int64_t n, int k)
{
    if (n <= 0 || k < 1 || k > LOB_MAX_K) return 8;
    const int64_t rpc = lob_rows_per_chunk(n);
    return (n + rpc - 1) / rpc * k * (int64_t)sizeof(double);
}

HPCLA_API int hpcla_lobpcg_residual_f64(hpcla_comm_t *comm, const double *X, int64_t ldx, const double *AX, int64_t ldax,
                                        const double *theta_dev, const double *minv, double *W, int64_t ldw, double *W2,
                                        int64_t ldw2, int64_t n, int k, double *rn2_dev, void *work, void *stream)
{
    if (k < 1 || k > LOB_MAX_K) return set_error(HPCLA_ERR_INVALID, "lobpcg_residual: needs 1 <= k <= 16");
    if (n < 0 || ldx < k || ldax < k || ldw < k || (W2 && ldw2 < k))
        return set_error(HPCLA_ERR_INVALID, "lobpcg_residual: negative size, or a pitch shorter than k");
    if (!rn2_dev || (reinterpret_cast<uintptr_t>(rn2_dev) & 7))
        return set_error(HPCLA_ERR_INVALID, "lobpcg_residual: null or misaligned sums");
    hipStream_t s = as_stream(stream);
    if (n == 0) {                                    // no local rows: the partial is zero, the rank still reduces
        HPCLA_CHECK_HIP(hipMemsetAsync(rn2_dev, 0, (size_t)k * sizeof(double), s));
    } else {
        if (!X || !AX || !W || !theta_dev || !work) return set_error(HPCLA_ERR_INVALID, "lobpcg_residual: null X / AX / W / theta / work");
        if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(AX) | reinterpret_cast<uintptr_t>(W) |
             reinterpret_cast<uintptr_t>(W2) | reinterpret_cast<uintptr_t>(theta_dev) | reinterpret_cast<uintptr_t>(minv) |
             reinterpret_cast<uintptr_t>(work)) & 7)
            return set_error(HPCLA_ERR_INVALID, "lobpcg_residual: every array must be 8-byte aligned");
        const int64_t rpc = lob_rows_per_chunk(n);
        const int64_t nchunks = (n + rpc - 1) / rpc;
        HPCLA_CHECK_GRID(nchunks, "lobpcg_residual");
        double *partial = static_cast<double *>(work);
        const bool vec = lob_even_aligned(X, ldx) && lob_even_aligned(AX, ldax) && lob_even_aligned(W, ldw) && lob_even_aligned(W2, ldw2);
        if (vec)
            lobpcg_residual_kernel<true><<<(unsigned)nchunks, LOB_THREADS, 0, s>>>(X, ldx, AX, ldax, theta_dev, minv, W, ldw, W2,
                                                                                  ldw2, n, k, rpc, partial);
        else
            lobpcg_residual_kernel<false><<<(unsigned)nchunks, LOB_THREADS, 0, s>>>(X, ldx, AX, ldax, theta_dev, minv, W, ldw, W2,
                                                                                   ldw2, n, k, rpc, partial);
        HPCLA_CHECK_LAUNCH();
        lobpcg_residual_stage2<<<1, LOB_THREADS, 0, s>>>(partial, nchunks, k, rn2_dev);
        HPCLA_CHECK_LAUNCH();
    }
    if (comm) return allreduce_on(comm, rn2_dev, k, 0, stream);
    return HPCLA_OK;
}

HPCLA_API int64_t hpcla_lobpcg_gen_work_bytes(int64_t n, int k)
{
    if (n <= 0 || k < 1 || k > LOB_MAX_K) return 8;
    const int64_t rpc = lob_rows_per_chunk(n);
    return (n + rpc - 1) / rpc * LOB_GEN_SUMS * k * (int64_t)sizeof(double);
}

HPCLA_API int hpcla_lobpcg_residual_gen_f64(hpcla_comm_t *comm, const double *AX, int64_t ldax, const double *BX, int64_t ldbx,
                                            const double *theta_dev, const double *minv, const double *bdiag, double *W,
                                            int64_t ldw, double *W2, int64_t ldw2, double *BW, int64_t ldbw, int64_t n, int k,
                                            double *sums_dev, void *work, void *stream)
{
    if (k < 1 || k > LOB_MAX_K) return set_error(HPCLA_ERR_INVALID, "lobpcg_residual_gen: needs 1 <= k <= 16");
    if (n < 0 || ldax < k || ldbx < k || ldw < k || (W2 && ldw2 < k) || (BW && ldbw < k))
        return set_error(HPCLA_ERR_INVALID, "lobpcg_residual_gen: negative size, or a pitch shorter than k");
    if (!sums_dev || (reinterpret_cast<uintptr_t>(sums_dev) & 7))
        return set_error(HPCLA_ERR_INVALID, "lobpcg_residual_gen: null or misaligned sums");
    hipStream_t s = as_stream(stream);
    if (n == 0) {                                    // no local rows: the partials are zero, the rank still reduces
        for (int q = 0; q < LOB_GEN_SUMS; ++q)
            HPCLA_CHECK_HIP(hipMemsetAsync(sums_dev + q * LOB_MAX_K, 0, (size_t)k * sizeof(double), s));
    } else {
        if (!AX || !BX || !W || !theta_dev || !work)
            return set_error(HPCLA_ERR_INVALID, "lobpcg_residual_gen: null AX / BX / W / theta / work");
        if (!bdiag != !BW)
            return set_error(HPCLA_ERR_INVALID, "lobpcg_residual_gen: bdiag and BW are given together or not at all");
        if ((reinterpret_cast<uintptr_t>(AX) | reinterpret_cast<uintptr_t>(BX) | reinterpret_cast<uintptr_t>(W) |
             reinterpret_cast<uintptr_t>(W2) | reinterpret_cast<uintptr_t>(BW) | reinterpret_cast<uintptr_t>(theta_dev) |
             reinterpret_cast<uintptr_t>(minv) | reinterpret_cast<uintptr_t>(bdiag) | reinterpret_cast<uintptr_t>(work)) & 7)
            return set_error(HPCLA_ERR_INVALID, "lobpcg_residual_gen: every array must be 8-byte aligned");
        const int64_t rpc = lob_rows_per_chunk(n);
        const int64_t nchunks = (n + rpc - 1) / rpc;
        HPCLA_CHECK_GRID(nchunks, "lobpcg_residual_gen");
        double *partial = static_cast<double *>(work);
        const bool vec = lob_even_aligned(AX, ldax) && lob_even_aligned(BX, ldbx) && lob_even_aligned(W, ldw) &&
                         lob_even_aligned(W2, ldw2) && lob_even_aligned(BW, ldbw);
        if (vec)
            lobpcg_residual_gen_kernel<true><<<(unsigned)nchunks, LOB_THREADS, 0, s>>>(AX, ldax, BX, ldbx, theta_dev, minv, bdiag, W,
                                                                                      ldw, W2, ldw2, BW, ldbw, n, k, rpc, partial);
        else
            lobpcg_residual_gen_kernel<false><<<(unsigned)nchunks, LOB_THREADS, 0, s>>>(AX, ldax, BX, ldbx, theta_dev, minv, bdiag, W,
                                                                                       ldw, W2, ldw2, BW, ldbw, n, k, rpc, partial);
        HPCLA_CHECK_LAUNCH();
        lobpcg_residual_gen_stage2<<<1, LOB_THREADS, 0, s>>>(partial, nchunks, k, sums_dev);
        HPCLA_CHECK_LAUNCH();
    }
    if (comm) return allreduce_on(comm, sums_dev, LOB_GEN_SUMS * LOB_MAX_K, 0, stream);
    return HPCLA_OK;
}

HPCLA_API int hpcla_lobpcg_combine_f64(double *S, int64_t lds, double *AS, int64_t ldas, const double *C_dev, int k, int c_rest,
                                       int64_t n, void *stream)
{
    if (k < 1 || k > LOB_MAX_K) return set_error(HPCLA_ERR_INVALID, "lobpcg_combine: needs 1 <= k <= 16");
    if (c_rest != 0 && c_rest != k && c_rest != 2 * k)
        return set_error(HPCLA_ERR_INVALID, "lobpcg_combine: c_rest must be 0, k or 2k");
    const int64_t need = c_rest ? 3 * (int64_t)k : k;    // P' is written at columns 2k .. 3k-1
    if (n < 0 || lds < need || (AS && ldas < need))
        return set_error(HPCLA_ERR_INVALID, "lobpcg_combine: negative size, or a pitch shorter than the block (k, or 3k with c_rest > 0)");
    if (!C_dev) return set_error(HPCLA_ERR_INVALID, "lobpcg_combine: null C");
    if (n == 0) return HPCLA_OK;
    if (!S) return set_error(HPCLA_ERR_INVALID, "lobpcg_combine: null S");
    if ((reinterpret_cast<uintptr_t>(S) | reinterpret_cast<uintptr_t>(AS) | reinterpret_cast<uintptr_t>(C_dev)) & 7)
        return set_error(HPCLA_ERR_INVALID, "lobpcg_combine: S, AS and C must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const int kt = k <= 4 ? 4 : (k <= 8 ? 8 : 16);
    const int rows = LOB_THREADS / (kt / LOB_JPL);       // rows of a workgroup's tile: 256, 128 or 64
    const int64_t tiles = (n + rows - 1) / rows;
    HPCLA_CHECK_GRID(tiles * 2, "lobpcg_combine");
    const unsigned grid = (unsigned)(AS ? tiles * 2 : tiles);
    const size_t shmem = ((size_t)LOB_C_DOUBLES + (size_t)rows * (size_t)((c_rest ? 3 * k : k) | 1)) * sizeof(double);
    const bool vec = !(k & 1) && lob_even_aligned(S, lds) && lob_even_aligned(AS, ldas);
#define HPCLA_COMBINE(KT)                                                                                                     \
    if (vec) lobpcg_combine_kernel<KT, true><<<grid, LOB_THREADS, shmem, s>>>(S, lds, AS, ldas, C_dev, k, c_rest, n);         \
    else lobpcg_combine_kernel<KT, false><<<grid, LOB_THREADS, shmem, s>>>(S, lds, AS, ldas, C_dev, k, c_rest, n)
    if (kt == 4) { HPCLA_COMBINE(4); }
    else if (kt == 8) { HPCLA_COMBINE(8); }
    else { HPCLA_COMBINE(16); }
#undef HPCLA_COMBINE
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}
