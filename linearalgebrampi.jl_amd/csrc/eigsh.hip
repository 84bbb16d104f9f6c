// eigsh.hip -- the restart of thick-restart Lanczos (hp.eigsh): V[:, 0:p] <- V[:, 0:m] * S in ONE pass over the basis.
//
// The basis is the GMRES one: columns of n doubles at an even pitch ldv, so every column is 16-byte aligned.  S is the small
// right factor (m x p, m <= 64 rows: the Ritz vectors of the projected matrix the host keeps), column j at S + j*m.  The
// product is tall and skinny with the small factor on the right: a row of the result needs that row of V and all of S, nothing
// else, so a lane owns rows outright:
//   * the lane loads all m inputs of its rows into registers BEFORE it stores anything -- the in-place form is then safe
//     without a second buffer (V carries no __restrict__: the stores alias the loads on purpose);
//   * lanes walk down a column, so the loads and the in-place stores are coalesced (8 or 16 bytes per lane);
//   * S is the same for every lane: it is indexed by the loop counters alone, the compiler reads it through the scalar unit
//     into SGPRs (s_load_dwordx*) and the multiplies take it as their scalar operand -- no LDS, no barrier, no per-lane load;
//   * acc = row[0]*S[0,j];  acc = acc + row[i]*S[i,j], i ascending: separately rounded (-ffp-contract=off), the order
//     tests/_eigsh_cases.py restates.
// m is a runtime value; the register tile is a template parameter MT = ceil(m/16)*16 in {16, 32, 48, 64}, and the loops over
// it are fully unrolled (a runtime-indexed register array would go to scratch): whole chunks of 16 columns run unguarded, so
// their coefficients arrive in one batch of scalar loads; the last, partial chunk runs as unguarded blocks of 8, 4, 2 and 1
// columns chosen by wave-uniform branches on the remainder, so no coefficient waits behind a branch of its own.  Up to
// MT = 32 a lane owns TWO rows as double2 (64 or 128 VGPRs of row data) and the odd last row is a one-row launch of the
// scalar form; at MT = 48 and 64 it owns one row (96, 128 VGPRs of row data): two rows there would be 192 / 256 VGPRs and
// one wave per SIMD.
// Bytes per row, in place: read m columns, write p, move the last column: 8 (m + p) + 16.  No loop waits on memory another
// workgroup writes; there is no inter-workgroup communication at all.
#include "common.h"

namespace hpcla {

constexpr int ROT_THREADS = 256;
constexpr int EIGSH_MAX_NCV = 64;

// one row (R = 1) or two adjacent rows (R = 2, a double2 at an even row) per lane
template <int R> struct RotRows;
template <> struct RotRows<1> {
    double x;
    __device__ __forceinline__ void load(const double *p) { x = *p; }
    __device__ __forceinline__ void store(double *p) const { *p = x; }
    __device__ __forceinline__ void store_strided(double *p, int64_t rs) const { p[0] = x; }
    __device__ __forceinline__ void first(const RotRows &a, double s) { x = a.x * s; }
    __device__ __forceinline__ void add(const RotRows &a, double s) { x = x + a.x * s; }
};
template <> struct RotRows<2> {
    double2 v;
    __device__ __forceinline__ void load(const double *p) { v = *reinterpret_cast<const double2 *>(p); }
    __device__ __forceinline__ void store(double *p) const { *reinterpret_cast<double2 *>(p) = v; }
    __device__ __forceinline__ void store_strided(double *p, int64_t rs) const
    {
        p[0] = v.x;
        p[rs] = v.y;
    }
    __device__ __forceinline__ void first(const RotRows &a, double s)
    {
        v.x = a.v.x * s;
        v.y = a.v.y * s;
    }
    __device__ __forceinline__ void add(const RotRows &a, double s)
    {
        v.x = v.x + a.v.x * s;
        v.y = v.y + a.v.y * s;
    }
};

// acc += row[i] * Sj[i] for i in [START, START + LEN), i ascending; column 0 is the caller's (acc starts from it)
template <int START, int LEN, int R>
__device__ __forceinline__ void rot_block(RotRows<R> &acc, const RotRows<R> *row, const double *__restrict__ Sj)
{
#pragma unroll
    for (int i = START; i < START + LEN; ++i)
        if (i > 0) acc.add(row[i], Sj[i]);
}

// the last, partial chunk: columns [START, START + rem), rem < 2 LEN, as unguarded blocks of LEN, LEN / 2, ... 1 columns.  Every
// index is a compile-time constant and every block's coefficients are one batch of scalar loads; rem is wave-uniform
template <int START, int LEN, int R>
__device__ __forceinline__ void rot_tail(RotRows<R> &acc, const RotRows<R> *row, const double *__restrict__ Sj, int rem)
{
    if constexpr (LEN >= 1) {
        if (rem >= LEN) {
            rot_block<START, LEN, R>(acc, row, Sj);
            rot_tail<START + LEN, LEN / 2, R>(acc, row, Sj, rem - LEN);
        } else {
            rot_tail<START, LEN / 2, R>(acc, row, Sj, rem);
        }
    }
}

// columns [C0, m): whole chunks of 16 (their 16 coefficients in one batch of scalar loads), then the partial one
template <int C0, int MT, int R>
__device__ __forceinline__ void rot_chunks(RotRows<R> &acc, const RotRows<R> *row, const double *__restrict__ Sj, int m)
{
    if constexpr (C0 < MT) {
        if (C0 + 16 <= m) {
            rot_block<C0, 16, R>(acc, row, Sj);
            rot_chunks<C0 + 16, MT, R>(acc, row, Sj, m);
        } else if (C0 < m) {
            rot_tail<C0, 8, R>(acc, row, Sj, m - C0);
        }
    }
}

// rows r .. r + R - 1 (r + R <= n; r even when R = 2).  out == NULL: in place
template <int MT, int R>
__device__ __forceinline__ void rotate_rows(double *V, int64_t ldv, int m, int p, const double *__restrict__ S, int move_last,
                                            double *out, int64_t ors, int64_t ocs, int64_t r)
{
    RotRows<R> row[MT], last;
#pragma unroll
    for (int i = 0; i < MT; ++i)
        if (i < m) row[i].load(V + (int64_t)i * ldv + r);
    if (move_last) last.load(V + (int64_t)m * ldv + r);
    for (int j = 0; j < p; ++j) {
        const double *Sj = S + (int64_t)j * m;
        RotRows<R> acc;
        acc.first(row[0], Sj[0]);
        int mj = m;                                              // opaque per column: the chunk tests below are then scalar compares
        asm volatile("" : "+s"(mj));                             // made in the loop, not lane masks kept (and spilled) across it
        if (mj == MT) rot_block<0, MT, R>(acc, row, Sj);          // a full tile: straight-line, the loads of a chunk under the last one's arithmetic
        else rot_chunks<0, MT, R>(acc, row, Sj, mj);
        if (out) acc.store_strided(out + r * ors + (int64_t)j * ocs, ors);
        else acc.store(V + (int64_t)j * ldv + r);
    }
    if (move_last) last.store(V + (int64_t)p * ldv + r);
}

template <int MT, int R>
__global__ __launch_bounds__(ROT_THREADS) void eigsh_rotate_kernel(double *V, int64_t ldv, int m, int p,
                                                                   const double *__restrict__ S, int move_last, double *out,
                                                                   int64_t ors, int64_t ocs, int64_t n)
{
    const int64_t g = (int64_t)blockIdx.x * ROT_THREADS + threadIdx.x;
    if (g < n / R) rotate_rows<MT, R>(V, ldv, m, p, S, move_last, out, ors, ocs, g * R);
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int hpcla_eigsh_rotate_f64(double *V, int64_t ldv, int m, int p, const double *S_dev, int move_last, double *out,
                                     int64_t out_row_stride, int64_t out_col_stride, int64_t n, void *stream)
{
    if (n < 0 || ldv < n || (ldv & 1)) return set_error(HPCLA_ERR_INVALID, "eigsh_rotate: negative size, or an odd or short pitch");
    if (m < 1 || m > EIGSH_MAX_NCV || p < 1 || p > m) return set_error(HPCLA_ERR_INVALID, "eigsh_rotate: needs 1 <= p <= m <= 64");
    if (!S_dev) return set_error(HPCLA_ERR_INVALID, "eigsh_rotate: null S");
    if (out && (move_last || out_row_stride < 1 || out_col_stride < 1))
        return set_error(HPCLA_ERR_INVALID, "eigsh_rotate: the out-of-place form takes positive strides and moves no column");
    if (n == 0) return HPCLA_OK;
    if (!V) return set_error(HPCLA_ERR_INVALID, "eigsh_rotate: null basis");
    if ((reinterpret_cast<uintptr_t>(V) & 15) || (reinterpret_cast<uintptr_t>(S_dev) & 7) || (reinterpret_cast<uintptr_t>(out) & 7))
        return set_error(HPCLA_ERR_INVALID, "eigsh_rotate: the basis must be 16-byte aligned, S and out 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const int tile = (m + 15) / 16;
    const int64_t grid = ((tile <= 2 ? n / 2 : n) + ROT_THREADS - 1) / ROT_THREADS;
    HPCLA_CHECK_GRID(grid, "eigsh_rotate");
    // the double2 tiles leave the odd last row to a one-row launch of the scalar form (row n - 1 seen as a basis of one row)
    double *Vt = V + (n - 1), *outt = out ? out + (n - 1) * out_row_stride : nullptr;
#define HPCLA_ROTATE(MT, R)                                                                                                   \
    if (grid) eigsh_rotate_kernel<MT, R><<<(unsigned)grid, ROT_THREADS, 0, s>>>(V, ldv, m, p, S_dev, move_last, out,          \
                                                                               out_row_stride, out_col_stride, n);            \
    if (R == 2 && (n & 1))                                                                                                    \
        eigsh_rotate_kernel<MT, 1><<<1, 64, 0, s>>>(Vt, ldv, m, p, S_dev, move_last, outt, out_row_stride, out_col_stride, 1)
    switch (tile) {
    case 1: HPCLA_ROTATE(16, 2); break;
    case 2: HPCLA_ROTATE(32, 2); break;
    case 3: HPCLA_ROTATE(48, 1); break;
    default: HPCLA_ROTATE(64, 1); break;
    }
#undef HPCLA_ROTATE
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}
