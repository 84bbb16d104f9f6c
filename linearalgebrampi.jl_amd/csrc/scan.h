// scan.h -- the library's one device-wide exclusive scan: three phases over blocks of SCAN_B elements (per-block sums,
// one block scanning the sums, per-block scan + emit).  What is scanned and what is written are functors, so the same three
// kernels serve the presence bitmap of the column-space construction (construct.hip) and the row counts / presence bitmap
// of the submatrix extraction (submatrix.hip):
//   Load:  int64_t operator()(int64_t i) const              -- the value of element i, i in [0, n)
//   Emit:  void operator()(int64_t i, int64_t before, int64_t v) const -- `before` = sum of the values of elements < i
#pragma once
#include "common.h"

namespace hpcla {

constexpr int SCAN_T = 256;
constexpr int SCAN_E = 4;                       // elements per thread
constexpr int SCAN_B = SCAN_T * SCAN_E;         // 1024 elements per block

static inline int64_t scan_blocks(int64_t n) { return (n + SCAN_B - 1) / SCAN_B; }

// block-local exclusive scan of one value per thread; writes the block total
__device__ __forceinline__ int64_t block_exclusive_scan(int64_t v, int64_t *s_warp, int64_t *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_warp[w] = inc;
    __syncthreads();
    int64_t base = 0;
    for (int k = 0; k < w; ++k) base += s_warp[k];
    if (total) {
        int64_t tot = 0;
        for (int k = 0; k < SCAN_T / 64; ++k) tot += s_warp[k];
        *total = tot;
    }
    __syncthreads();
    return base + inc - v;
}

template <typename Load>
__global__ __launch_bounds__(SCAN_T) void scan_phase1_kernel(Load load, int64_t n, int64_t *__restrict__ block_sums)
{
    __shared__ int64_t s_warp[SCAN_T / 64];
    const int64_t b0 = (int64_t)blockIdx.x * SCAN_B + (int64_t)threadIdx.x * SCAN_E;
    int64_t v = 0;
#pragma unroll
    for (int k = 0; k < SCAN_E; ++k)
        if (b0 + k < n) v += load(b0 + k);
    int64_t tot;
    (void)block_exclusive_scan(v, s_warp, &tot);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

// one block scans all block sums in place (exclusive), returns the grand total in total[0]
static __global__ __launch_bounds__(SCAN_T) void scan_phase2_kernel(int64_t *__restrict__ block_sums, int64_t nb,
                                                                    int64_t *__restrict__ total)
{
    __shared__ int64_t s_warp[SCAN_T / 64];
    __shared__ int64_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int64_t c = 0; c < nb; c += SCAN_T) {
        const int64_t i = c + threadIdx.x;
        const int64_t v = i < nb ? block_sums[i] : 0;
        int64_t tot;
        const int64_t ex = block_exclusive_scan(v, s_warp, &tot);
        const int64_t carry = s_carry;
        if (i < nb) block_sums[i] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = s_carry;
}

// emit(i, sum of the elements before i, element i) for every i in [0, n)
template <typename Load, typename Emit>
__global__ __launch_bounds__(SCAN_T) void scan_phase3_kernel(Load load, int64_t n, const int64_t *__restrict__ block_offs,
                                                             Emit emit)
{
    __shared__ int64_t s_warp[SCAN_T / 64];
    const int64_t b0 = (int64_t)blockIdx.x * SCAN_B + (int64_t)threadIdx.x * SCAN_E;
    int64_t f[SCAN_E];
    int64_t v = 0;
#pragma unroll
    for (int k = 0; k < SCAN_E; ++k) {
        f[k] = b0 + k < n ? load(b0 + k) : 0;
        v += f[k];
    }
    int64_t pos = block_offs[blockIdx.x] + block_exclusive_scan(v, s_warp, nullptr);
#pragma unroll
    for (int k = 0; k < SCAN_E; ++k) {
        if (b0 + k < n) {
            emit(b0 + k, pos, f[k]);
            pos += f[k];
        }
    }
}

// The three phases on stream s: block_sums holds scan_blocks(n) words, total one.  n >= 1.
template <typename Load, typename Emit>
static int exclusive_scan(Load load, int64_t n, Emit emit, int64_t *block_sums, int64_t *total, hipStream_t s)
{
    const int64_t nb = scan_blocks(n);
    HPCLA_CHECK_GRID(nb, "scan");
    scan_phase1_kernel<Load><<<(uint32_t)nb, SCAN_T, 0, s>>>(load, n, block_sums);
    HPCLA_CHECK_LAUNCH();
    scan_phase2_kernel<<<1, SCAN_T, 0, s>>>(block_sums, nb, total);
    HPCLA_CHECK_LAUNCH();
    scan_phase3_kernel<Load, Emit><<<(uint32_t)nb, SCAN_T, 0, s>>>(load, n, block_sums, emit);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

}  // namespace hpcla
