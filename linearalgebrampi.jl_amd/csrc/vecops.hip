// vecops.hip -- dot / norm reductions and fused vector updates (the CG building blocks).
//
// Replaces the reference's local BLAS dot/nrm2 + host MPI Allreduce (src/vectors.jl:758-812) and
// its allocating elementwise ops / broadcast (src/vectors.jl:868-903, 944-964, 1203-1226).
// All kernels are pure HBM streams (16-byte loads, grid-stride, <= 4096 blocks).  Reductions are
// two-stage and deterministic: fixed grid, per-block partial -> one block sums the partials in
// index order; the scalar stays on the device so a CG iteration never synchronises the host.
// Bytes per element: dot 16 (8 for x.x), nrm2sq/asum/amax 8, axpy/xpay 24, scale 16, axpby 24.
#include <stdlib.h>

#include "comm_internal.h"
#include "solver_slots.h"

namespace hpcla {

constexpr int RT = 256;            // threads per reduction block
constexpr int MAX_PARTIALS = 2048; // upper bound of stage-1 blocks

enum RedOp { RED_DOT = 0, RED_SQ = 1, RED_ABS = 2, RED_MAX = 3, RED_SUM = 4, RED_POW = 5, RED_MAXV = 6, RED_PROD = 7 };
// RED_MAX: max |x| (identity 0);  RED_MAXV: max x (identity -inf; min x = -max(-x) with negate = 1);
// RED_PROD: product (identity 1)

template <int OP>
__device__ __forceinline__ double red_map(double a, double b, double p = 0.0)
{
    if (OP == RED_POW) return pow(fabs(a), p);
    if (OP == RED_MAXV) return p != 0.0 ? -a : a;          // p doubles as the "negate" flag
    if (OP == RED_DOT) return a * b;
    if (OP == RED_SQ) return a * a;
    if (OP == RED_SUM || OP == RED_PROD) return a;
    return fabs(a);
}
template <int OP>
__device__ __forceinline__ double red_comb(double s, double v)
{
    // NaN-propagating like Julia's maximum / norm(., Inf) (src/vectors.jl:769-772): a plain `v > s ? v : s` never selects
    // a NaN v, which would let rows poisoned by an expired halo wait (halo_poison) pass as a finite maximum
    if (OP == RED_MAX || OP == RED_MAXV) return (v > s || v != v) ? v : s;
    if (OP == RED_PROD) return s * v;
    return s + v;
}

template <int OP>
__device__ __forceinline__ double block_reduce(double v)
{
    __shared__ double s_w[RT / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = red_comb<OP>(v, __shfl_down(v, off, 64));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_w[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        r = s_w[0];
#pragma unroll
        for (int i = 1; i < RT / 64; ++i) r = red_comb<OP>(r, s_w[i]);
    }
    return r;   // valid in thread 0
}

template <int OP>
__global__ __launch_bounds__(RT) void reduce_stage1(const double *__restrict__ x,
                                                    const double *__restrict__ y, int64_t n,
                                                    double *__restrict__ partial, double p = 0.0)
{
    // 16-byte loads on the aligned body, scalar tail
    double acc = OP == RED_MAXV ? -__builtin_huge_val() : (OP == RED_PROD ? 1.0 : 0.0);
    const int64_t n2 = n / 2;
    const double2 *x2 = reinterpret_cast<const double2 *>(x);
    const double2 *y2 = reinterpret_cast<const double2 *>(OP == RED_DOT ? y : x);
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 a = x2[i];
        double2 b = a;
        if (OP == RED_DOT) b = y2[i];
        acc = red_comb<OP>(acc, red_map<OP>(a.x, b.x, p));
        acc = red_comb<OP>(acc, red_map<OP>(a.y, b.y, p));
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        acc = red_comb<OP>(acc, red_map<OP>(x[n - 1], OP == RED_DOT ? y[n - 1] : x[n - 1], p));
    const double r = block_reduce<OP>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

template <int OP>
__global__ __launch_bounds__(RT) void reduce_stage2(const double *__restrict__ partial, int np,
                                                    double *__restrict__ out)
{
    double acc = OP == RED_MAXV ? -__builtin_huge_val() : (OP == RED_PROD ? 1.0 : 0.0);
    for (int i = threadIdx.x; i < np; i += RT) acc = red_comb<OP>(acc, partial[i]);
    const double r = block_reduce<OP>(acc);
    if (threadIdx.x == 0) out[0] = r;
}

static inline int reduce_grid(int64_t n)
{
    int64_t g = (n / 2 + RT * 4 - 1) / (RT * 4);   // >= 4 double2 per thread
    if (g < 1) g = 1;
    if (g > MAX_PARTIALS) g = MAX_PARTIALS;
    return (int)g;
}

int allreduce_on(hpcla_comm_t *comm, double *buf, int64_t count, int op, void *stream);  // comm.hip

template <int OP>
static int reduce_impl(hpcla_comm_t *comm, const double *x, const double *y, int64_t n,
                       double *out_dev, void *work, void *stream, double p = 0.0)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "reduce: negative size");
    if (!out_dev || !work) return set_error(HPCLA_ERR_INVALID, "reduce: null out/work");
    if (n > 0 && (!x || (OP == RED_DOT && !y)))
        return set_error(HPCLA_ERR_INVALID, "reduce: null input");
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (OP == RED_DOT && (reinterpret_cast<uintptr_t>(y) & 15)))
        return set_error(HPCLA_ERR_INVALID, "reduce: inputs must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    if (g == 1) {
        // short vectors: the single stage-1 workgroup's partial IS the result (one launch, not two)
        reduce_stage1<OP><<<1, RT, 0, s>>>(x, y, n, out_dev, p);
        HPCLA_CHECK_LAUNCH();
    } else {
        reduce_stage1<OP><<<g, RT, 0, s>>>(x, y, n, partial, p);
        HPCLA_CHECK_LAUNCH();
        reduce_stage2<OP == RED_POW ? RED_SUM : OP><<<1, RT, 0, s>>>(partial, g, out_dev);
        HPCLA_CHECK_LAUNCH();
    }
    if (comm) return allreduce_on(comm, out_dev, 1, (OP == RED_MAX || OP == RED_MAXV) ? 1 : (OP == RED_PROD ? 2 : 0), stream);
    return HPCLA_OK;
}

// sum `np` per-workgroup partials (deterministic two-stage tree) into out[0]; `scratch` holds
// MAX_PARTIALS doubles.  Used by the fused SpMV+dot (spmv.hip) and the fused CG update.
int reduce_partials_sum(const double *partial, int64_t np, double *scratch, double *out, void *stream)
{
    if (np < 0) return set_error(HPCLA_ERR_INVALID, "reduce_partials: bad count");
    hipStream_t s = as_stream(stream);
    if (np <= 4 * RT) {
        reduce_stage2<RED_SUM><<<1, RT, 0, s>>>(partial, (int)np, out);
    } else {
        const int g = reduce_grid(np);
        reduce_stage1<RED_SUM><<<g, RT, 0, s>>>(partial, nullptr, np, scratch);
        HPCLA_CHECK_LAUNCH();
        reduce_stage2<RED_SUM><<<1, RT, 0, s>>>(scratch, g, out);
    }
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// fused CG update (replaces two broadcasts + one norm of src/vectors.jl:1203-1226, 758-765):
//   a = alpha * *num / *den ;  x += a*p ;  r -= a*Ap ;  partial[block] = sum r_new^2
__global__ __launch_bounds__(RT) void cg_update_kernel(double alpha, const double *__restrict__ num,
                                                       const double *__restrict__ den,
                                                       const double *__restrict__ p,
                                                       const double *__restrict__ Ap,
                                                       double *__restrict__ x, double *__restrict__ r,
                                                       int64_t n, double *__restrict__ partial)
{
    double a = alpha;
    if (num) a = a * num[0];
    if (den) a = a / den[0];
    const int64_t n2 = n / 2;
    const double2 *p2 = reinterpret_cast<const double2 *>(p);
    const double2 *q2 = reinterpret_cast<const double2 *>(Ap);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    double2 *r2 = reinterpret_cast<double2 *>(r);
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 pv = p2[i], qv = q2[i];
        double2 xv = x2[i], rv = r2[i];
        xv.x = xv.x + a * pv.x;
        xv.y = xv.y + a * pv.y;
        rv.x = rv.x - a * qv.x;
        rv.y = rv.y - a * qv.y;
        x2[i] = xv;
        r2[i] = rv;
        acc = acc + rv.x * rv.x;
        acc = acc + rv.y * rv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        x[j] = x[j] + a * p[j];
        const double rn = r[j] - a * Ap[j];
        r[j] = rn;
        acc = acc + rn * rn;
    }
    const double s = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__device__ __forceinline__ double dev_scalar(double alpha, const double *num, const double *den)
{
    double a = alpha;
    if (num) a = a * num[0];
    if (den) a = a / den[0];
    return a;
}

// The same CG iteration with the x update DEFERRED to the direction update (both read p_k, so p is read
// once instead of twice: SpMV + 64 B/row of vector traffic instead of 72).  Per element the operations and
// their operands are those of cg_update_kernel + update_kernel<1>: same bits.
//   residual:  a = alpha * *num / *den ;  r -= a*Ap ;  partial[block] = sum r_new^2
//   direction: a as above, b = beta * *bnum / *bden ;  x += a*p ;  p = r + b*p
typedef double v2d_nt __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 nt_load2(const double2 *p)
{
    const v2d_nt t = __builtin_nontemporal_load(reinterpret_cast<const v2d_nt *>(p));
    double2 r;
    r.x = t.x; r.y = t.y;
    return r;
}
__device__ __forceinline__ void nt_store2(double2 v, double2 *p)
{
    v2d_nt t;
    t.x = v.x; t.y = v.y;
    __builtin_nontemporal_store(t, reinterpret_cast<v2d_nt *>(p));
}

// Cache policy of the CG update kernels (round 4; HPCLA_CG_NT bit mask, default 7 = all three): a vector that is not touched again
// before ~2-3 GB of other traffic has passed is loaded / stored NON-TEMPORALLY, so that L2 and the 256 MiB Infinity Cache
// keep the vectors the next kernels re-read (p: gathered by the SpMV; r, Ap: read by the next update).
//   bit 0 (1): x in the direction update (load + store) -- measured -4.4 % per CG iteration
//   bit 1 (2): r load in the direction update (next use: the residual update behind the next SpMV)
//   bit 2 (4): Ap load in the residual update (its last use)
// Config 4's slab, ms per iteration, two alternating rounds of processes on one box (profiles/r04_cg_nontemporal_x.log):
// mask 0: 0.5250 / 0.5233, 1: 0.4997 / 0.5041, 3: 0.4951 / 0.4957, 5: 0.5022 / 0.5006, 7: 0.4903 / 0.4899 (-6.5 %).
// Same operations on the same operands: same bits.
template <bool NTQ>
__global__ __launch_bounds__(RT) void cg_residual_kernel(double alpha, const double *__restrict__ num,
                                                         const double *__restrict__ den,
                                                         const double *__restrict__ Ap, double *__restrict__ r,
                                                         int64_t n, double *__restrict__ partial)
{
    const double a = dev_scalar(alpha, num, den);
    const int64_t n2 = n / 2;
    const double2 *q2 = reinterpret_cast<const double2 *>(Ap);
    double2 *r2 = reinterpret_cast<double2 *>(r);
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 qv = NTQ ? nt_load2(q2 + i) : q2[i];
        double2 rv = r2[i];
        rv.x = rv.x - a * qv.x;
        rv.y = rv.y - a * qv.y;
        r2[i] = rv;
        acc = acc + rv.x * rv.x;
        acc = acc + rv.y * rv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double rn = r[j] - a * Ap[j];
        r[j] = rn;
        acc = acc + rn * rn;
    }
    const double s = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

template <bool NTX, bool NTR>
__global__ __launch_bounds__(256) void cg_direction_kernel(double alpha, const double *__restrict__ num,
                                                           const double *__restrict__ den, double beta,
                                                           const double *__restrict__ bnum,
                                                           const double *__restrict__ bden,
                                                           const double *__restrict__ r, double *__restrict__ x,
                                                           double *__restrict__ p, int64_t n)
{
    const double a = dev_scalar(alpha, num, den);
    const double b = dev_scalar(beta, bnum, bden);
    const int64_t n2 = n / 2;
    const double2 *r2 = reinterpret_cast<const double2 *>(r);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    double2 *p2 = reinterpret_cast<double2 *>(p);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n2; i += stride) {
        const double2 rv = NTR ? nt_load2(r2 + i) : r2[i];
        const double2 pv0 = p2[i];
        double2 xv = NTX ? nt_load2(x2 + i) : x2[i], pv = pv0;
        xv.x = xv.x + a * pv.x;
        xv.y = xv.y + a * pv.y;
        pv.x = rv.x + b * pv.x;
        pv.y = rv.y + b * pv.y;
        if (NTX) nt_store2(xv, x2 + i); else x2[i] = xv;
        p2[i] = pv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double pj = p[j];
        x[j] = x[j] + a * pj;
        p[j] = r[j] + b * pj;
    }
}

// ---- gated, diagonally preconditioned forms of the pair above (the solver hpcla_pcg_iterations_*) ----------------
// Iteration j (1-based over the whole solve) of preconditioned CG with z = dinv .* r NEVER stored:
//   residual:  a = *num / *den (rz_{j-1} / pAp) ;  r -= a*Ap ;  partials of sum r^2 and sum r*(dinv*r)
//   direction: a as above, b = *bnum / *bden (rz_j / rz_{j-1}) ;  x += a*p ;  p = dinv*r + b*p
// 32 (residual) + 48 (direction) = 80 B per row against the plain pair's 64: dinv is read twice, like a stored z would be
// written once and read once.  PRECOND = false (dinv == NULL, the identity) has no dinv load and no multiply: grid, body,
// tail, accumulation order and cache policy are those of cg_residual_kernel / cg_direction_kernel, hence their bits.
//
// The solve's state lives on the device so that the host looks at it once per chunk of iterations, and the iterations
// already enqueued behind the deciding one are no-ops (continuing at full accuracy drives rz and pAp to 0/0):
//   state[0] done_iter   the iteration the solve ended on (meaningful once status != 0)
//   state[1] status      0 running, 1 converged (sum r_j^2 <= thr at j = done_iter), 2 breakdown (!(pAp > 0) at done_iter + 1)
//   state[2] thr         max(rtol |b|, atol)^2 as a double, written by the caller
// The residual kernel runs while status == 0 and pAp > 0; the direction kernel while status == 0, and once more for
// done_iter >= j: the x update of the converging iteration is deferred into it.  One uniform load per workgroup.
constexpr int64_t PCG_RUNNING = 0, PCG_CONVERGED = 1, PCG_BREAKDOWN = 2;
constexpr int PCG_STATE_WORDS = 4;

template <bool NTQ, bool PRECOND>
__global__ __launch_bounds__(RT) void pcg_residual_kernel(const double *__restrict__ num, const double *__restrict__ den,
                                                          const double *__restrict__ Ap, const double *__restrict__ dinv,
                                                          double *__restrict__ r, int64_t n, const int64_t *__restrict__ state,
                                                          double *__restrict__ partial_rr, double *__restrict__ partial_rz)
{
    if (state[1] != PCG_RUNNING || !(den[0] > 0.0)) return;      // frozen, or gate A (recorded by pcg_stage2_kernel)
    const double a = dev_scalar(1.0, num, den);
    const int64_t n2 = n / 2;
    const double2 *q2 = reinterpret_cast<const double2 *>(Ap);
    const double2 *d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *r2 = reinterpret_cast<double2 *>(r);
    double acc = 0.0, acz = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 qv = NTQ ? nt_load2(q2 + i) : q2[i];
        double2 rv = r2[i];
        rv.x = rv.x - a * qv.x;
        rv.y = rv.y - a * qv.y;
        r2[i] = rv;
        acc = acc + rv.x * rv.x;
        acc = acc + rv.y * rv.y;
        if (PRECOND) {
            const double2 dv = d2[i];
            acz = acz + rv.x * (dv.x * rv.x);
            acz = acz + rv.y * (dv.y * rv.y);
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double rn = r[j] - a * Ap[j];
        r[j] = rn;
        acc = acc + rn * rn;
        if (PRECOND) acz = acz + rn * (dinv[j] * rn);
    }
    const double s = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) partial_rr[blockIdx.x] = s;
    if (PRECOND) {
        __syncthreads();                                         // block_reduce's LDS slots are reused
        const double z = block_reduce<RED_SUM>(acz);
        if (threadIdx.x == 0) partial_rz[blockIdx.x] = z;
    }
}

__device__ __forceinline__ void pcg_gate_b(const double *pair, int64_t iter, int64_t *state)
{
    if (pair[0] <= reinterpret_cast<const double *>(state)[2]) {
        state[0] = iter;
        state[1] = PCG_CONVERGED;
    }
}

// second stage of both sums (reduce_stage2<RED_SUM>'s order), one workgroup; records gate A, and gate B where no
// all-reduce stands between this kernel and the pair (gate_b != 0)
template <bool PRECOND>
__global__ __launch_bounds__(RT) void pcg_stage2_kernel(const double *__restrict__ partial_rr,
                                                        const double *__restrict__ partial_rz, int np,
                                                        const double *__restrict__ den, int64_t iter, int gate_b,
                                                        int64_t *__restrict__ state, double *__restrict__ pair)
{
    if (state[1] != PCG_RUNNING) return;
    if (!(den[0] > 0.0)) {                                       // gate A: also catches a NaN pAp
        if (threadIdx.x == 0) {
            state[0] = iter - 1;
            state[1] = PCG_BREAKDOWN;
        }
        return;
    }
    double acc = 0.0, acz = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) acc = acc + partial_rr[i];
    const double rr = block_reduce<RED_SUM>(acc);
    double rz = rr;
    if (PRECOND) {
        for (int i = threadIdx.x; i < np; i += RT) acz = acz + partial_rz[i];
        __syncthreads();
        rz = block_reduce<RED_SUM>(acz);
    }
    if (threadIdx.x == 0) {
        pair[0] = rr;
        pair[1] = rz;
        if (gate_b) pcg_gate_b(pair, iter, state);
    }
}

__global__ void pcg_gate_b_kernel(const double *__restrict__ pair, int64_t iter, int64_t *__restrict__ state)
{
    if (threadIdx.x == 0 && state[1] == PCG_RUNNING) pcg_gate_b(pair, iter, state);
}

template <bool NTX, bool NTR, bool PRECOND>
__global__ __launch_bounds__(256) void pcg_direction_kernel(const double *__restrict__ num, const double *__restrict__ den,
                                                            const double *__restrict__ bnum, const double *__restrict__ bden,
                                                            const double *__restrict__ r, const double *__restrict__ dinv,
                                                            double *__restrict__ x, double *__restrict__ p, int64_t n,
                                                            int64_t iter, const int64_t *__restrict__ state)
{
    const int64_t status = state[1];
    if (!(status == PCG_RUNNING || (status == PCG_CONVERGED && state[0] >= iter))) return;
    const double a = dev_scalar(1.0, num, den);
    const double b = dev_scalar(1.0, bnum, bden);
    const int64_t n2 = n / 2;
    const double2 *r2 = reinterpret_cast<const double2 *>(r);
    const double2 *d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    double2 *p2 = reinterpret_cast<double2 *>(p);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n2; i += stride) {
        double2 rv = NTR ? nt_load2(r2 + i) : r2[i];
        const double2 pv0 = p2[i];
        double2 xv = NTX ? nt_load2(x2 + i) : x2[i], pv = pv0;
        if (PRECOND) {
            const double2 dv = d2[i];
            rv.x = dv.x * rv.x;
            rv.y = dv.y * rv.y;
        }
        xv.x = xv.x + a * pv.x;
        xv.y = xv.y + a * pv.y;
        pv.x = rv.x + b * pv.x;
        pv.y = rv.y + b * pv.y;
        if (NTX) nt_store2(xv, x2 + i); else x2[i] = xv;
        p2[i] = pv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double pj = p[j];
        double zj = r[j];
        if (PRECOND) zj = dinv[j] * zj;
        x[j] = x[j] + a * pj;
        p[j] = zj + b * pj;
    }
}

// ---- gated BiCGStab steps (the solver hpcla_bicgstab_iterations_*; right preconditioning, K = identity or dinv .*) ----
// Iteration j (1-based over the whole solve); v = A ph and t = A sh are the SpMV's, ungated.  Bytes per row, plain / with dinv:
//   bicg_dot   rv = rhat.v                                               read rhat, v                            16 / 16
//   bicg_s     a = rho/rv;  s = r - a*v  [sh = dinv*s]                   read r, v [dinv], write s [sh]          24 / 40
//   bicg_tts   ts = t.s, tt = t.t, ss = s.s in ONE pass                  read t, s                               16 / 16
//   bicg_xr    w = ts/tt;  x = (x + a*ph) + w*sh;  r = s - w*t;          read x, ph, s [sh], t, rhat, write x, r 56 / 64
//              rho' = rhat.r, rr = r.r      (half-step form: x = x + a*ph only, 24 B)
//   bicg_p     b = (rho'/rho)*(a/w);  p = r + b*(p - w*v)  [ph = dinv*p] read r, p, v [dinv], write p [ph]       32 / 48
// 144 B per row and iteration next to the two SpMVs (184 with dinv); composed from dot / axpy / xpay it is about 216 B, five
// host read-backs and about 13 launches.  PRECOND = false has no dinv load and no multiply: ph IS p and sh IS s (one load).
// Every kernel forms a, w, b from the same device doubles with the expressions above, so each has the same bits wherever it
// is used; multiplies and adds are rounded separately, in the order written.
//
// The state is PCG's (done_iter, status, thr, reserved) with one more status, set by gate S and reported as converged:
//   3 converged at the half step: ss_j <= thr at j = done_iter; bicg_xr of that iteration then runs in its half-step form
// Gates, in this order (each needs status == 0):
//   A  after rv:            !(rho != 0 && rv != 0), NaN included      -> breakdown, done_iter = j - 1
//   S  after (ts, tt, ss):  ss <= thr                                 -> status 3, done_iter = j; the history pair's first entry
//                                                                        receives ss from bicg_xr's gate, BEHIND the pair's
//                                                                        all-reduce (written before it, N ranks would sum it)
//   T                       !(tt > 0)                                 -> breakdown, done_iter = j - 1 (x and r untouched)
//   B  after (rr, rho'):    rr <= thr                                 -> converged, done_iter = j
//   O                       ts == 0 (w = 0: the next direction is 0/0) -> breakdown, done_iter = j (x and r are updated)
// Cache policy: x in bicg_xr (HPCLA_CG_NT bit 0) and t in bicg_xr (bit 2: its last use) are not touched again within the
// iteration and go non-temporally, as x and Ap do in the CG pair; every other vector is re-read by the next kernels.
constexpr int64_t BICG_CONVERGED_HALF = 3;
constexpr int BICG_PARTIAL_ARRAYS = 3;

__device__ __forceinline__ bool bicg_nonzero(double a) { return fabs(a) > 0.0; }     // false for +-0 and for NaN

__device__ __forceinline__ void bicg_gate_a(double rho, double rv, int64_t iter, int64_t *state)
{
    if (!(bicg_nonzero(rho) && bicg_nonzero(rv))) {
        state[0] = iter - 1;
        state[1] = PCG_BREAKDOWN;
    }
}

__device__ __forceinline__ void bicg_gate_st(const double *triple, int64_t iter, int64_t *state)
{
    if (triple[2] <= reinterpret_cast<const double *>(state)[2]) {
        state[0] = iter;
        state[1] = BICG_CONVERGED_HALF;
    } else if (!(triple[1] > 0.0)) {
        state[0] = iter - 1;
        state[1] = PCG_BREAKDOWN;
    }
}

// also the half step's history entry: triple[2] = ss, already all-reduced, stored where no all-reduce follows
__device__ __forceinline__ void bicg_gate_bo(double *pair, const double *triple, int64_t iter, int64_t *state)
{
    if (state[1] == BICG_CONVERGED_HALF && state[0] == iter) {
        pair[0] = triple[2];
        return;
    }
    if (state[1] != PCG_RUNNING) return;
    const double ts = triple[0];
    if (pair[0] <= reinterpret_cast<const double *>(state)[2]) {
        state[0] = iter;
        state[1] = PCG_CONVERGED;
    } else if (ts == 0.0) {
        state[0] = iter;
        state[1] = PCG_BREAKDOWN;
    }
}

// step 2, first stage: reduce_stage1<RED_DOT>'s grid, body, tail and order, gated
__global__ __launch_bounds__(RT) void bicg_dot_kernel(const double *__restrict__ rhat, const double *__restrict__ v, int64_t n,
                                                      const int64_t *__restrict__ state, double *__restrict__ partial)
{
    if (state[1] != PCG_RUNNING) return;
    const int64_t n2 = n / 2;
    const double2 *a2 = reinterpret_cast<const double2 *>(rhat);
    const double2 *b2 = reinterpret_cast<const double2 *>(v);
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 a = a2[i], b = b2[i];
        acc = acc + a.x * b.x;
        acc = acc + a.y * b.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) acc = acc + rhat[n - 1] * v[n - 1];
    const double r = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// second stage of rv (reduce_stage2<RED_SUM>'s order), one workgroup; records gate A where no all-reduce follows (gate != 0)
__global__ __launch_bounds__(RT) void bicg_dot_stage2_kernel(const double *__restrict__ partial, int np,
                                                             const double *__restrict__ rho, int64_t iter, int gate,
                                                             int64_t *__restrict__ state, double *__restrict__ rv_out)
{
    if (state[1] != PCG_RUNNING) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) acc = acc + partial[i];
    const double rv = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) {
        rv_out[0] = rv;
        if (gate) bicg_gate_a(rho[0], rv, iter, state);
    }
}

__global__ void bicg_gate_a_kernel(const double *__restrict__ rho, const double *__restrict__ rv, int64_t iter,
                                   int64_t *__restrict__ state)
{
    if (threadIdx.x == 0 && state[1] == PCG_RUNNING) bicg_gate_a(rho[0], rv[0], iter, state);
}

// step 3
template <bool PRECOND>
__global__ __launch_bounds__(256) void bicg_s_kernel(const double *__restrict__ rho, const double *__restrict__ rv,
                                                     const double *__restrict__ r, const double *__restrict__ v,
                                                     const double *__restrict__ dinv, double *__restrict__ s,
                                                     double *__restrict__ sh, int64_t n, const int64_t *__restrict__ state)
{
    if (state[1] != PCG_RUNNING) return;
    const double rh = rho[0], den = rv[0];
    if (!(bicg_nonzero(rh) && bicg_nonzero(den))) return;         // gate A (recorded by the second stage of rv)
    const double a = rh / den;
    const int64_t n2 = n / 2;
    const double2 *r2 = reinterpret_cast<const double2 *>(r);
    const double2 *v2 = reinterpret_cast<const double2 *>(v);
    const double2 *d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *s2 = reinterpret_cast<double2 *>(s);
    double2 *h2 = reinterpret_cast<double2 *>(sh);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n2; i += stride) {
        const double2 rw = r2[i], vv = v2[i];
        double2 sv;
        sv.x = rw.x - a * vv.x;
        sv.y = rw.y - a * vv.y;
        s2[i] = sv;
        if (PRECOND) {
            const double2 dv = d2[i];
            double2 hv;
            hv.x = dv.x * sv.x;
            hv.y = dv.y * sv.y;
            h2[i] = hv;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double sj = r[j] - a * v[j];
        s[j] = sj;
        if (PRECOND) sh[j] = dinv[j] * sj;
    }
}

// step 5, first stage: the three sums in one pass over t and s
__global__ __launch_bounds__(RT) void bicg_tts_kernel(const double *__restrict__ t, const double *__restrict__ s, int64_t n,
                                                      const int64_t *__restrict__ state, double *__restrict__ partial_ts,
                                                      double *__restrict__ partial_tt, double *__restrict__ partial_ss)
{
    if (state[1] != PCG_RUNNING) return;
    const int64_t n2 = n / 2;
    const double2 *t2 = reinterpret_cast<const double2 *>(t);
    const double2 *s2 = reinterpret_cast<const double2 *>(s);
    double ats = 0.0, att = 0.0, ass = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 tv = t2[i], sv = s2[i];
        ats = ats + tv.x * sv.x;
        ats = ats + tv.y * sv.y;
        att = att + tv.x * tv.x;
        att = att + tv.y * tv.y;
        ass = ass + sv.x * sv.x;
        ass = ass + sv.y * sv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double tj = t[n - 1], sj = s[n - 1];
        ats = ats + tj * sj;
        att = att + tj * tj;
        ass = ass + sj * sj;
    }
    const double a = block_reduce<RED_SUM>(ats);
    if (threadIdx.x == 0) partial_ts[blockIdx.x] = a;
    __syncthreads();                                             // block_reduce's LDS slots are reused
    const double b = block_reduce<RED_SUM>(att);
    if (threadIdx.x == 0) partial_tt[blockIdx.x] = b;
    __syncthreads();
    const double c = block_reduce<RED_SUM>(ass);
    if (threadIdx.x == 0) partial_ss[blockIdx.x] = c;
}

// second stage of the triple, one workgroup; records gates S and T where no all-reduce follows (gate != 0)
__global__ __launch_bounds__(RT) void bicg_tts_stage2_kernel(const double *__restrict__ partial_ts,
                                                             const double *__restrict__ partial_tt,
                                                             const double *__restrict__ partial_ss, int np, int64_t iter,
                                                             int gate, int64_t *__restrict__ state,
                                                             double *__restrict__ triple)
{
    if (state[1] != PCG_RUNNING) return;
    double ats = 0.0, att = 0.0, ass = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) ats = ats + partial_ts[i];
    const double ts = block_reduce<RED_SUM>(ats);
    for (int i = threadIdx.x; i < np; i += RT) att = att + partial_tt[i];
    __syncthreads();
    const double tt = block_reduce<RED_SUM>(att);
    for (int i = threadIdx.x; i < np; i += RT) ass = ass + partial_ss[i];
    __syncthreads();
    const double ss = block_reduce<RED_SUM>(ass);
    if (threadIdx.x == 0) {
        triple[0] = ts;
        triple[1] = tt;
        triple[2] = ss;
        if (gate) bicg_gate_st(triple, iter, state);
    }
}

__global__ void bicg_gate_st_kernel(const double *__restrict__ triple, int64_t iter, int64_t *__restrict__ state)
{
    if (threadIdx.x == 0 && state[1] == PCG_RUNNING) bicg_gate_st(triple, iter, state);
}

// step 6, first stage.  PRECOND = false: sh is s, loaded once
template <bool NTX, bool NTT, bool PRECOND>
__global__ __launch_bounds__(RT) void bicg_xr_kernel(const double *__restrict__ rho, const double *__restrict__ rv,
                                                     const double *__restrict__ ts, const double *__restrict__ tt,
                                                     const double *__restrict__ ph, const double *__restrict__ sh,
                                                     const double *__restrict__ s, const double *__restrict__ t,
                                                     const double *__restrict__ rhat, double *__restrict__ x,
                                                     double *__restrict__ r, int64_t n, int64_t iter,
                                                     const int64_t *__restrict__ state, double *__restrict__ partial_rr,
                                                     double *__restrict__ partial_rho)
{
    const int64_t status = state[1];
    const bool half = status == BICG_CONVERGED_HALF && state[0] == iter;
    if (!(status == PCG_RUNNING || half)) return;
    const double a = rho[0] / rv[0];
    const int64_t n2 = n / 2;
    const double2 *p2 = reinterpret_cast<const double2 *>(ph);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    if (half) {                                                  // gate S fired at this iteration: x = x + a*ph, nothing else
        for (; i < n2; i += stride) {
            const double2 pv = p2[i];
            double2 xv = NTX ? nt_load2(x2 + i) : x2[i];
            xv.x = xv.x + a * pv.x;
            xv.y = xv.y + a * pv.y;
            if (NTX) nt_store2(xv, x2 + i); else x2[i] = xv;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = x[n - 1] + a * ph[n - 1];
        return;
    }
    const double w = ts[0] / tt[0];
    const double2 *h2 = reinterpret_cast<const double2 *>(sh);
    const double2 *s2 = reinterpret_cast<const double2 *>(s);
    const double2 *t2 = reinterpret_cast<const double2 *>(t);
    const double2 *q2 = reinterpret_cast<const double2 *>(rhat);
    double2 *r2 = reinterpret_cast<double2 *>(r);
    double arr = 0.0, arho = 0.0;
    for (; i < n2; i += stride) {
        const double2 pv = p2[i], sv = s2[i], qv = q2[i];
        const double2 tv = NTT ? nt_load2(t2 + i) : t2[i];
        double2 hv = sv;
        if (PRECOND) hv = h2[i];
        double2 xv = NTX ? nt_load2(x2 + i) : x2[i], rw;
        xv.x = (xv.x + a * pv.x) + w * hv.x;
        xv.y = (xv.y + a * pv.y) + w * hv.y;
        rw.x = sv.x - w * tv.x;
        rw.y = sv.y - w * tv.y;
        if (NTX) nt_store2(xv, x2 + i); else x2[i] = xv;
        r2[i] = rw;
        arr = arr + rw.x * rw.x;
        arr = arr + rw.y * rw.y;
        arho = arho + qv.x * rw.x;
        arho = arho + qv.y * rw.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double sj = s[j];
        const double hj = PRECOND ? sh[j] : sj;
        x[j] = (x[j] + a * ph[j]) + w * hj;
        const double rn = sj - w * t[j];
        r[j] = rn;
        arr = arr + rn * rn;
        arho = arho + rhat[j] * rn;
    }
    const double c = block_reduce<RED_SUM>(arr);
    if (threadIdx.x == 0) partial_rr[blockIdx.x] = c;
    __syncthreads();                                             // block_reduce's LDS slots are reused
    const double d = block_reduce<RED_SUM>(arho);
    if (threadIdx.x == 0) partial_rho[blockIdx.x] = d;
}

// second stage of (rr, rho'), one workgroup; records gates B and O where no all-reduce follows (gate != 0).  For the half
// step of this iteration there are no sums: the gate only stores ss as the pair's first entry
__global__ __launch_bounds__(RT) void bicg_xr_stage2_kernel(const double *__restrict__ partial_rr,
                                                            const double *__restrict__ partial_rho, int np,
                                                            const double *__restrict__ triple, int64_t iter, int gate,
                                                            int64_t *__restrict__ state, double *__restrict__ pair)
{
    if (state[1] != PCG_RUNNING) {
        if (gate && threadIdx.x == 0) bicg_gate_bo(pair, triple, iter, state);
        return;
    }
    double arr = 0.0, arho = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) arr = arr + partial_rr[i];
    const double rr = block_reduce<RED_SUM>(arr);
    for (int i = threadIdx.x; i < np; i += RT) arho = arho + partial_rho[i];
    __syncthreads();
    const double rho_new = block_reduce<RED_SUM>(arho);
    if (threadIdx.x == 0) {
        pair[0] = rr;
        pair[1] = rho_new;
        if (gate) bicg_gate_bo(pair, triple, iter, state);
    }
}

__global__ void bicg_gate_bo_kernel(double *__restrict__ pair, const double *__restrict__ triple, int64_t iter,
                                    int64_t *__restrict__ state)
{
    if (threadIdx.x == 0) bicg_gate_bo(pair, triple, iter, state);
}

// step 7
template <bool PRECOND>
__global__ __launch_bounds__(256) void bicg_p_kernel(const double *__restrict__ rho_new, const double *__restrict__ rho,
                                                     const double *__restrict__ rv, const double *__restrict__ ts,
                                                     const double *__restrict__ tt, const double *__restrict__ r,
                                                     const double *__restrict__ v, const double *__restrict__ dinv,
                                                     double *__restrict__ p, double *__restrict__ ph, int64_t n,
                                                     const int64_t *__restrict__ state)
{
    if (state[1] != PCG_RUNNING) return;
    const double a = rho[0] / rv[0];
    const double w = ts[0] / tt[0];
    const double b = (rho_new[0] / rho[0]) * (a / w);
    const int64_t n2 = n / 2;
    const double2 *r2 = reinterpret_cast<const double2 *>(r);
    const double2 *v2 = reinterpret_cast<const double2 *>(v);
    const double2 *d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *p2 = reinterpret_cast<double2 *>(p);
    double2 *h2 = reinterpret_cast<double2 *>(ph);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n2; i += stride) {
        const double2 rw = r2[i], vv = v2[i];
        double2 pv = p2[i];
        pv.x = rw.x + b * (pv.x - w * vv.x);
        pv.y = rw.y + b * (pv.y - w * vv.y);
        p2[i] = pv;
        if (PRECOND) {
            const double2 dv = d2[i];
            double2 hv;
            hv.x = dv.x * pv.x;
            hv.y = dv.y * pv.y;
            h2[i] = hv;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double pj = r[j] + b * (p[j] - w * v[j]);
        p[j] = pj;
        if (PRECOND) ph[j] = dinv[j] * pj;
    }
}

// ---- gated LSQR steps (the solver hpcla_lsqr_iterations_*: min |A x - b|^2 + damp^2 |x|^2 for a rectangular A) -------------
// Golub-Kahan bidiagonalisation on A (m x n) and At with NO vector ever normalised in memory: uh and vh are kept unnormalised
// next to their norms beta and alpha, and the scalings ride in the passes that read the vectors anyway (two normalisation
// passes, 16 (m + n) bytes per row and column, are not made).  Iteration j (1-based over the whole solve); tu = A vh and
// tv = At uh are the SpMV's, ungated.  Bytes per row (u) or column (v, xw):
//   lsqr_u    uh = tu / alpha - (alpha / beta) uh;  uu = uh.uh                    read tu, uh, write uh            24
//   lsqr_v    beta' = sqrt(uu);  vh = tv / beta' - (beta' / alpha) vh;  vv = vh.vh  read tv, vh, write vh            24
//             gate U  uu == 0: vh is left alone and vv = 0 (exact termination: the step ends the solve)
//   step      one thread, behind vv's all-reduce; alpha' = sqrt(vv):
//             anorm2 += (alpha^2 + beta'^2) + damp^2
//             rhobar1 = sqrt(rhobar^2 + damp^2);  psi = (damp / rhobar1) phibar;  phibar = (rhobar / rhobar1) phibar;  res2 += psi^2
//             rho = sqrt(rhobar1^2 + beta'^2);  c = rhobar1 / rho;  s = beta' / rho;  theta = s alpha';  rhobar = -c alpha'
//             phi = c phibar;  phibar = s phibar;  t1 = phi / rho;  t2 = theta / rho
//             rn2 = phibar^2 + res2;  arn = alpha' |s phi|;  pair = (rn2, arn^2)
//             gates, in order:  !(rn2 and arn finite)                -> breakdown, done_iter = j - 1
//                               rn2 <= thr                           -> converged, done_iter = j
//                               arn^2 <= (ntol2 anorm2) rn2          -> least squares (status 3), done_iter = j
//             alpha = alpha';  beta = beta'
//   lsqr_xw   x = x + t1 w;  w = vh / alpha - t2 w                                read x, w, vh, write x, w        40
//             (x only, 24 B, in the iteration that stopped: status 1 or 3 and done_iter == j)
// 24 m + 64 n bytes per iteration next to the two SpMVs, two all-reduces; composed from norm / scale / axpy it is about
// 48 m + 96 n and four host read-backs.  Divides, multiplies and subtractions are rounded separately, in the order written.
// The state is PCG's (done_iter, status, thr, ntol2): thr = max(rtol |b|, atol)^2 and ntol2 = ntol^2 as doubles.
// The scalars live in LSQR_SCALARS doubles at these slots (damp is the caller's; the others are read and written here):
enum LsqrSlot {
    LSQR_ALPHA = 0, LSQR_BETA = 1, LSQR_UU = 2, LSQR_VV = 3, LSQR_PHIBAR = 4, LSQR_RHOBAR = 5, LSQR_RES2 = 6, LSQR_ANORM2 = 7,
    LSQR_T1 = 8, LSQR_T2 = 9, LSQR_RHO = 10, LSQR_C = 11, LSQR_S = 12, LSQR_THETA = 13, LSQR_PHI = 14, LSQR_RN2 = 15,
    LSQR_ARN = 16, LSQR_DAMP = 17, LSQR_SCALARS = 24
};
constexpr int64_t LSQR_LEAST_SQUARES = 3;
// Cache policy: tu in lsqr_u and tv in lsqr_v (HPCLA_CG_NT bit 2: their last use) and x in lsqr_xw (bit 0) are not touched
// again within the iteration and go non-temporally; uh, vh and w are re-read by the next SpMV or kernel.

__device__ __forceinline__ bool lsqr_finite(double a) { return fabs(a) < __builtin_huge_val(); }     // false for NaN too

template <bool NTQ>
__global__ __launch_bounds__(RT) void lsqr_u_kernel(const double *__restrict__ scal, const double *__restrict__ tu,
                                                    double *__restrict__ uh, int64_t n, const int64_t *__restrict__ state,
                                                    double *__restrict__ partial)
{
    if (state[1] != PCG_RUNNING) return;
    const double alpha = scal[LSQR_ALPHA];
    const double g = alpha / scal[LSQR_BETA];
    const int64_t n2 = n / 2;
    const double2 *t2 = reinterpret_cast<const double2 *>(tu);
    double2 *u2 = reinterpret_cast<double2 *>(uh);
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 tv = NTQ ? nt_load2(t2 + i) : t2[i];
        double2 uv = u2[i];
        uv.x = tv.x / alpha - g * uv.x;
        uv.y = tv.y / alpha - g * uv.y;
        u2[i] = uv;
        acc = acc + uv.x * uv.x;
        acc = acc + uv.y * uv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double un = tu[j] / alpha - g * uh[j];
        uh[j] = un;
        acc = acc + un * un;
    }
    const double r = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// second stage of uu (reduce_stage2<RED_SUM>'s order), one workgroup
__global__ __launch_bounds__(RT) void lsqr_u_stage2_kernel(const double *__restrict__ partial, int np,
                                                           const int64_t *__restrict__ state, double *__restrict__ scal)
{
    if (state[1] != PCG_RUNNING) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) acc = acc + partial[i];
    const double uu = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) scal[LSQR_UU] = uu;
}

template <bool NTQ>
__global__ __launch_bounds__(RT) void lsqr_v_kernel(const double *__restrict__ scal, const double *__restrict__ tv,
                                                    double *__restrict__ vh, int64_t n, const int64_t *__restrict__ state,
                                                    double *__restrict__ partial)
{
    if (state[1] != PCG_RUNNING) return;
    const double uu = scal[LSQR_UU];
    if (uu == 0.0) return;                                       // gate U (vv = 0 is the second stage's)
    const double beta = sqrt(uu);
    const double g = beta / scal[LSQR_ALPHA];
    const int64_t n2 = n / 2;
    const double2 *t2 = reinterpret_cast<const double2 *>(tv);
    double2 *v2 = reinterpret_cast<double2 *>(vh);
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 tw = NTQ ? nt_load2(t2 + i) : t2[i];
        double2 vv = v2[i];
        vv.x = tw.x / beta - g * vv.x;
        vv.y = tw.y / beta - g * vv.y;
        v2[i] = vv;
        acc = acc + vv.x * vv.x;
        acc = acc + vv.y * vv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double vn = tv[j] / beta - g * vh[j];
        vh[j] = vn;
        acc = acc + vn * vn;
    }
    const double r = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// the scalar step of iteration `iter` and its gates; uu and vv are global sums here.  pair is not all-reduced afterwards
__device__ __forceinline__ void lsqr_step(double *scal, double *pair, int64_t iter, int64_t *state)
{
    const double alpha = scal[LSQR_ALPHA], damp = scal[LSQR_DAMP];
    const double beta1 = sqrt(scal[LSQR_UU]), alpha1 = sqrt(scal[LSQR_VV]);
    const double anorm2 = scal[LSQR_ANORM2] + ((alpha * alpha + beta1 * beta1) + damp * damp);
    double rhobar = scal[LSQR_RHOBAR], phibar = scal[LSQR_PHIBAR];
    const double rhobar1 = sqrt(rhobar * rhobar + damp * damp);
    const double psi = (damp / rhobar1) * phibar;
    phibar = (rhobar / rhobar1) * phibar;
    const double res2 = scal[LSQR_RES2] + psi * psi;
    const double rho = sqrt(rhobar1 * rhobar1 + beta1 * beta1);
    const double c = rhobar1 / rho;
    const double s = beta1 / rho;
    const double theta = s * alpha1;
    rhobar = -c * alpha1;
    const double phi = c * phibar;
    phibar = s * phibar;
    const double t1 = phi / rho;
    const double t2 = theta / rho;
    const double rn2 = phibar * phibar + res2;
    const double arn = alpha1 * fabs(s * phi);
    const double arn2 = arn * arn;
    scal[LSQR_ANORM2] = anorm2;
    scal[LSQR_RES2] = res2;
    scal[LSQR_RHO] = rho;
    scal[LSQR_C] = c;
    scal[LSQR_S] = s;
    scal[LSQR_THETA] = theta;
    scal[LSQR_RHOBAR] = rhobar;
    scal[LSQR_PHI] = phi;
    scal[LSQR_PHIBAR] = phibar;
    scal[LSQR_T1] = t1;
    scal[LSQR_T2] = t2;
    scal[LSQR_RN2] = rn2;
    scal[LSQR_ARN] = arn;
    scal[LSQR_ALPHA] = alpha1;
    scal[LSQR_BETA] = beta1;
    pair[0] = rn2;
    pair[1] = arn2;
    const double *lim = reinterpret_cast<const double *>(state);
    if (!(lsqr_finite(rn2) && lsqr_finite(arn))) {
        state[0] = iter - 1;
        state[1] = PCG_BREAKDOWN;
    } else if (rn2 <= lim[2]) {
        state[0] = iter;
        state[1] = PCG_CONVERGED;
    } else if (arn2 <= (lim[3] * anorm2) * rn2) {
        state[0] = iter;
        state[1] = LSQR_LEAST_SQUARES;
    }
}

// second stage of vv, one workgroup; gate U's vv = 0; the step where no all-reduce follows (pair != NULL)
__global__ __launch_bounds__(RT) void lsqr_v_stage2_kernel(const double *__restrict__ partial, int np, int64_t iter,
                                                           int64_t *__restrict__ state, double *__restrict__ scal,
                                                           double *__restrict__ pair)
{
    if (state[1] != PCG_RUNNING) return;
    double vv = 0.0;
    if (scal[LSQR_UU] != 0.0) {                                  // uniform; else gate U: the partials are stale
        double acc = 0.0;
        for (int i = threadIdx.x; i < np; i += RT) acc = acc + partial[i];
        vv = block_reduce<RED_SUM>(acc);
    }
    if (threadIdx.x == 0) {
        scal[LSQR_VV] = vv;
        if (pair) lsqr_step(scal, pair, iter, state);
    }
}

__global__ void lsqr_step_kernel(double *__restrict__ scal, double *__restrict__ pair, int64_t iter,
                                 int64_t *__restrict__ state)
{
    if (threadIdx.x == 0 && state[1] == PCG_RUNNING) lsqr_step(scal, pair, iter, state);
}

template <bool NTX>
__global__ __launch_bounds__(256) void lsqr_xw_kernel(const double *__restrict__ scal, const double *__restrict__ vh,
                                                      double *__restrict__ x, double *__restrict__ w, int64_t n, int64_t iter,
                                                      const int64_t *__restrict__ state)
{
    const int64_t status = state[1];
    const bool last = (status == PCG_CONVERGED || status == LSQR_LEAST_SQUARES) && state[0] == iter;
    if (!(status == PCG_RUNNING || last)) return;
    const double t1 = scal[LSQR_T1];
    const int64_t n2 = n / 2;
    const double2 *v2 = reinterpret_cast<const double2 *>(vh);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    double2 *w2 = reinterpret_cast<double2 *>(w);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (last) {                                                  // the iteration that stopped: x = x + t1 w, nothing else
        for (; i < n2; i += stride) {
            const double2 wv = w2[i];
            double2 xv = NTX ? nt_load2(x2 + i) : x2[i];
            xv.x = xv.x + t1 * wv.x;
            xv.y = xv.y + t1 * wv.y;
            if (NTX) nt_store2(xv, x2 + i); else x2[i] = xv;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) x[n - 1] = x[n - 1] + t1 * w[n - 1];
        return;
    }
    const double alpha = scal[LSQR_ALPHA], t2 = scal[LSQR_T2];
    for (; i < n2; i += stride) {
        const double2 vv = v2[i];
        double2 wv = w2[i];
        double2 xv = NTX ? nt_load2(x2 + i) : x2[i];
        xv.x = xv.x + t1 * wv.x;
        xv.y = xv.y + t1 * wv.y;
        wv.x = vv.x / alpha - t2 * wv.x;
        wv.y = vv.y / alpha - t2 * wv.y;
        if (NTX) nt_store2(xv, x2 + i); else x2[i] = xv;
        w2[i] = wv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double wj = w[j];
        x[j] = x[j] + t1 * wj;
        w[j] = vh[j] / alpha - t2 * wj;
    }
}

// ---- gated MINRES steps (the solver hpcla_minres_iterations_*: A x = b for a symmetric, possibly indefinite A) -------------
// Paige and Saunders' Lanczos recurrence with a positive definite diagonal preconditioner M = dinv .* (or the identity) and
// NO vector normalised in memory: the Lanczos vectors r1, r2 stay unnormalised next to their M-norms oldb, beta, y = M r2 is
// the SpMV's operand (r2 itself without M) and v = y / beta is never stored.  Two buffers each of r, w (and y with M) rotate by
// pointer: rn overwrites r1 (its last use), yn the y of the iteration before, the new w overwrites w1.  Iteration j (1-based
// over the whole solve); t = A y and yt = y.t are the SpMV's, ungated.  Bytes per row:
//   minres_r   alfa = yt / (beta beta)                                                          read t, r1, r2, write rn   32
//              rn = (t / beta - (alfa / beta) r2) - (beta / oldb) r1   (j = 1: no r1 term, r1 is only written: 24)
//              [ yn = dinv .* rn ];  bb = rn.yn                                      with M: + read dinv, write yn         48
//   step       one thread, behind bb's all-reduce:
//              gate N  !(bb >= 0), or bb or alfa not finite       -> breakdown, done_iter = j - 1, no scalar is written
//              beta' = sqrt(bb);  oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa
//              epsln = sn beta';  dbar = (-cs) beta';  gamma = sqrt(gbar gbar + beta' beta')
//              gate G  !(gamma > 0)                               -> breakdown, done_iter = j - 1, no scalar is written
//              cs = gbar / gamma;  sn = beta' / gamma;  phi = cs phibar;  phibar = sn phibar
//              pair = (phibar phibar, bb);  oldb = beta;  beta = beta'
//              gate C  phibar phibar <= thr                       -> converged, done_iter = j
//   minres_xw  w = ((y / oldb - oldeps w1) - delta w2) / gamma;  x = x + phi w        read y, w1, w2, x, write w, x        48
//              (y and oldb are this iteration's operand and its norm: minres_r left both alone; still runs for done_iter == j)
// 80 bytes per iteration next to the SpMV (96 with M: y is stored once so that xw does not read r2 and dinv, 8 bytes fewer than
// forming v from them), two all-reduces [yt], [bb]; composed from dot / norm / scale / axpy it is 176 and two host read-backs.
// beta' = 0 is the lucky termination: sn = 0, phibar = 0 and gate C ends the solve before anything is divided by beta'.
// Divides, multiplies, adds, subtractions and square roots are rounded separately, in the order written.
// The state is PCG's (done_iter, status, thr): thr = max(rtol sqrt(b.M b), atol)^2 as a double.
// The scalars live in MINRES_SCALARS doubles at the slots of MinresSlot (solver_slots.h: the iterations loop in solvers.hip names
// yt's slot too; yt is the SpMV's, the others are read and written here).
// Cache policy: t in minres_r (HPCLA_CG_NT bit 2: its last use) and x in minres_xw (bit 0) are not touched again within the
// iteration and go non-temporally; r, y and w are re-read by the next SpMV or kernel.

template <bool NTQ, bool PRECOND>
__global__ __launch_bounds__(RT) void minres_r_kernel(const double *__restrict__ scal, const double *__restrict__ t,
                                                      const double *__restrict__ r2, const double *__restrict__ dinv,
                                                      double *__restrict__ r1, double *__restrict__ yn, int64_t n, int64_t iter,
                                                      const int64_t *__restrict__ state, double *__restrict__ partial)
{
    if (state[1] != PCG_RUNNING) return;
    const double beta = scal[MINRES_BETA];
    const double alfa = scal[MINRES_YT] / (beta * beta);
    const double a = alfa / beta;
    const bool first = iter == 1;                                // no r1 term: r1 is only written
    const double c = first ? 0.0 : beta / scal[MINRES_OLDB];
    const int64_t n2 = n / 2;
    const double2 *t2 = reinterpret_cast<const double2 *>(t);
    const double2 *q2 = reinterpret_cast<const double2 *>(r2);
    const double2 *d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *p2 = reinterpret_cast<double2 *>(r1);
    double2 *y2 = reinterpret_cast<double2 *>(yn);
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 tv = NTQ ? nt_load2(t2 + i) : t2[i];
        const double2 qv = q2[i];
        double2 rn;
        rn.x = tv.x / beta - a * qv.x;
        rn.y = tv.y / beta - a * qv.y;
        if (!first) {
            const double2 pv = p2[i];
            rn.x = rn.x - c * pv.x;
            rn.y = rn.y - c * pv.y;
        }
        p2[i] = rn;
        if (PRECOND) {
            const double2 dv = d2[i];
            double2 yv;
            yv.x = dv.x * rn.x;
            yv.y = dv.y * rn.y;
            y2[i] = yv;
            acc = acc + rn.x * yv.x;
            acc = acc + rn.y * yv.y;
        } else {
            acc = acc + rn.x * rn.x;
            acc = acc + rn.y * rn.y;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        double rn = t[j] / beta - a * r2[j];
        if (!first) rn = rn - c * r1[j];
        r1[j] = rn;
        double yv = rn;
        if (PRECOND) {
            yv = dinv[j] * rn;
            yn[j] = yv;
        }
        acc = acc + rn * yv;
    }
    const double s = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the scalar step of iteration `iter` and its gates; yt and bb are global sums here.  pair is not all-reduced afterwards
__device__ __forceinline__ void minres_step(double *scal, double *pair, int64_t iter, int64_t *state)
{
    const double beta = scal[MINRES_BETA], bb = scal[MINRES_BB];
    const double alfa = scal[MINRES_YT] / (beta * beta);
    if (!(bb >= 0.0 && lsqr_finite(bb) && lsqr_finite(alfa))) {  // gate N (a NaN fails bb >= 0)
        state[0] = iter - 1;
        state[1] = PCG_BREAKDOWN;
        return;
    }
    const double cs = scal[MINRES_CS], sn = scal[MINRES_SN], dbar = scal[MINRES_DBAR], phibar = scal[MINRES_PHIBAR];
    const double betan = sqrt(bb);
    const double oldeps = scal[MINRES_EPSLN];
    const double delta = cs * dbar + sn * alfa;
    const double gbar = sn * dbar - cs * alfa;
    const double epsln = sn * betan;
    const double dbarn = (-cs) * betan;
    const double gamma = sqrt(gbar * gbar + betan * betan);
    if (!(gamma > 0.0)) {                                        // gate G: also catches a NaN gamma
        state[0] = iter - 1;
        state[1] = PCG_BREAKDOWN;
        return;
    }
    const double csn = gbar / gamma;
    const double snn = betan / gamma;
    const double phi = csn * phibar;
    const double phibarn = snn * phibar;
    const double res2 = phibarn * phibarn;
    scal[MINRES_ALFA] = alfa;
    scal[MINRES_OLDEPS] = oldeps;
    scal[MINRES_DELTA] = delta;
    scal[MINRES_GBAR] = gbar;
    scal[MINRES_EPSLN] = epsln;
    scal[MINRES_DBAR] = dbarn;
    scal[MINRES_GAMMA] = gamma;
    scal[MINRES_CS] = csn;
    scal[MINRES_SN] = snn;
    scal[MINRES_PHI] = phi;
    scal[MINRES_PHIBAR] = phibarn;
    scal[MINRES_OLDB] = beta;
    scal[MINRES_BETA] = betan;
    pair[0] = res2;
    pair[1] = bb;
    if (res2 <= reinterpret_cast<const double *>(state)[2]) {    // gate C
        state[0] = iter;
        state[1] = PCG_CONVERGED;
    }
}

// second stage of bb (reduce_stage2<RED_SUM>'s order), one workgroup; the step where no all-reduce follows (pair != NULL)
__global__ __launch_bounds__(RT) void minres_r_stage2_kernel(const double *__restrict__ partial, int np, int64_t iter,
                                                             int64_t *__restrict__ state, double *__restrict__ scal,
                                                             double *__restrict__ pair)
{
    if (state[1] != PCG_RUNNING) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) acc = acc + partial[i];
    const double bb = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) {
        scal[MINRES_BB] = bb;
        if (pair) minres_step(scal, pair, iter, state);
    }
}

__global__ void minres_step_kernel(double *__restrict__ scal, double *__restrict__ pair, int64_t iter,
                                   int64_t *__restrict__ state)
{
    if (threadIdx.x == 0 && state[1] == PCG_RUNNING) minres_step(scal, pair, iter, state);
}

template <bool NTX>
__global__ __launch_bounds__(256) void minres_xw_kernel(const double *__restrict__ scal, const double *__restrict__ y,
                                                        const double *__restrict__ w2, double *__restrict__ w1,
                                                        double *__restrict__ x, int64_t n, int64_t iter,
                                                        const int64_t *__restrict__ state)
{
    const int64_t status = state[1];
    if (!(status == PCG_RUNNING || (status == PCG_CONVERGED && state[0] == iter))) return;
    const double oldb = scal[MINRES_OLDB], oldeps = scal[MINRES_OLDEPS], delta = scal[MINRES_DELTA];
    const double gamma = scal[MINRES_GAMMA], phi = scal[MINRES_PHI];
    const int64_t n2 = n / 2;
    const double2 *y2 = reinterpret_cast<const double2 *>(y);
    const double2 *b2 = reinterpret_cast<const double2 *>(w2);
    double2 *a2 = reinterpret_cast<double2 *>(w1);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n2; i += stride) {
        const double2 yv = y2[i], bv = b2[i];
        double2 wv = a2[i];
        double2 xv = NTX ? nt_load2(x2 + i) : x2[i];
        wv.x = ((yv.x / oldb - oldeps * wv.x) - delta * bv.x) / gamma;
        wv.y = ((yv.y / oldb - oldeps * wv.y) - delta * bv.y) / gamma;
        xv.x = xv.x + phi * wv.x;
        xv.y = xv.y + phi * wv.y;
        a2[i] = wv;
        if (NTX) nt_store2(xv, x2 + i); else x2[i] = xv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        const double wj = ((y[j] / oldb - oldeps * w1[j]) - delta * w2[j]) / gamma;
        w1[j] = wj;
        x[j] = x[j] + phi * wj;
    }
}

// ---- gated GMRES(m) steps (the solver hpcla_gmres_iterations_*; right preconditioning, K = identity or dinv .*) ---------
// Inner step k (1-based over the whole solve), column j = (k - 1) mod m, c = j + 1 basis columns V_0 .. V_j at pitch ldv (even,
// so every column is 16-byte aligned); w = A z is the SpMV's, ungated (z is V_j without a preconditioner).  Classical
// Gram-Schmidt applied twice (CGS2).  Bytes per row:
//   gmres_dots     h[i] = V_i . w, i < c, tiles of GMRES_TILE columns        read w once per tile, c columns      8 c + 8 ceil(c/8)
//   gmres_update   w = ((w - h[0] V_0) - h[1] V_1) - ...  in ONE pass         read c columns, read and write w     8 c + 16
//                  (the second pass also emits the partials of w.w)
//   gmres_next     V_{j+1} = w / col_c  [z = dinv .* V_{j+1}]                read w [dinv], write V_{j+1} [z]     16 / 32
// dots, update, dots, update, next: 32 c + 48 + 16 ceil(c/8) per step (16 more with dinv) in 6 + 2 ceil(c/8) launches and no
// read-back; composed from dot and axpy it is 2 c dots at 16 and 2 c axpys at 24: 80 c, 4 c launches, 2 c + 1 read-backs.
//   gmres_xupdate  u = y[0] V_0;  u = u + y[i] V_i;  x = x + u  or  x + dinv .* u    once per cycle: 8 c + 16 [+ 8]
//   gmres_residual w = b - w (w holds A x), partials of w.w                  once per cycle: 24
// Every multiply, add, subtract, divide and sqrt is rounded separately, in the order written.  The accumulators of gmres_dots
// are a compile-time tile held in registers; a column's sum uses the grid, body, tail and order of reduce_stage1 whatever
// rides along, so it has the same bits for every c.
//
// The state is PCG's (done_iter, status, thr, reserved) with one more status, reported as converged:
//   3 converged at a restart: the true residual's w.w <= thr at k = done_iter (gate R); hist[k] then holds that w.w
// The small step (one thread, redundantly on every rank from all-reduced values) and its gates, each needing status == 0:
//   col[i] = h1[i] + h2[i];  col[c] = sqrt(nn);  the stored rotations i < j;  d = sqrt(col[j]^2 + col[j+1]^2)
//   D  !(d > 0), NaN included           -> breakdown, done_iter = k - 1; nothing of column j is stored
//   c_j, s_j, R[0..j, j], g[j], g[j+1];  hist[k] = g[j+1]^2
//   C  hist[k] <= thr                   -> converged, done_iter = k (a lucky breakdown, nn = 0, gives g[j+1] = 0 and ends here)
// Cache policy: x in gmres_xupdate goes non-temporally under HPCLA_CG_NT bit 0; basis columns are re-read every step and stay
// plain.
constexpr int64_t GMRES_CONVERGED_RESTART = 3;
constexpr int GMRES_TILE = AR_MAX;             // on purpose: one tile of sums is one window all-reduce
constexpr int GMRES_MAX_RESTART = 64;

// the small arrays of a solve, all in one buffer of gmres_small_layout(m, ...) doubles
struct GmresSmall {
    double *R, *cs, *sn, *g, *h1, *h2, *col, *y, *nn, *hn;   // R: m x m, column j at R + j m;  g, col: m + 1;  nn, hn: 1
};

static void gmres_small_offsets(int m, int64_t off[11])         // off[10]: the buffer's length
{
    const int64_t len[10] = {(int64_t)m * m, m, m, m + 1, m, m, m + 1, m, 1, 1};
    off[0] = 0;
    for (int i = 0; i < 10; ++i) off[i + 1] = off[i] + len[i];
}

static void gmres_small_layout(int m, double *base, GmresSmall *q)
{
    int64_t off[11];
    gmres_small_offsets(m, off);
    *q = GmresSmall{base + off[0], base + off[1], base + off[2], base + off[3], base + off[4],
                    base + off[5], base + off[6], base + off[7], base + off[8], base + off[9]};
}

__device__ void gmres_small_step(const GmresSmall &q, int j, int m, double nn, double *hist_k, int64_t iter, int64_t *state)
{
    const int c = j + 1;
    for (int i = 0; i < c; ++i) q.col[i] = q.h1[i] + q.h2[i];
    const double hn = sqrt(nn);
    q.col[c] = hn;
    q.hn[0] = hn;
    for (int i = 0; i < j; ++i) {
        const double ci = q.cs[i], si = q.sn[i], a = q.col[i], b = q.col[i + 1];
        const double t = ci * a + si * b;
        q.col[i + 1] = (-si) * a + ci * b;
        q.col[i] = t;
    }
    const double a = q.col[j], b = q.col[j + 1];
    const double d = sqrt(a * a + b * b);
    if (!(d > 0.0)) {                                            // gate D
        state[0] = iter - 1;
        state[1] = PCG_BREAKDOWN;
        return;
    }
    const double cj = a / d, sj = b / d;
    q.cs[j] = cj;
    q.sn[j] = sj;
    double *Rj = q.R + (int64_t)j * m;
    for (int i = 0; i < j; ++i) Rj[i] = q.col[i];
    Rj[j] = d;
    const double gj = q.g[j];
    const double gn = (-sj) * gj;
    q.g[j + 1] = gn;
    q.g[j] = cj * gj;
    const double e = gn * gn;
    hist_k[0] = e;
    if (e <= reinterpret_cast<const double *>(state)[2]) {       // gate C
        state[0] = iter;
        state[1] = PCG_CONVERGED;
    }
}

// gate R and the start of a cycle: beta = sqrt(rr), g = (beta, 0, ...).  hist[0] is the true residual's whatever the gate says
__device__ void gmres_restart_gate(const GmresSmall &q, int m, double rr, double *hist_k, int64_t iter, int64_t *state)
{
    if (rr <= reinterpret_cast<const double *>(state)[2]) {
        hist_k[0] = rr;
        state[0] = iter;
        state[1] = GMRES_CONVERGED_RESTART;
        return;
    }
    if (iter == 0) hist_k[0] = rr;
    const double beta = sqrt(rr);
    q.g[0] = beta;
    for (int i = 1; i <= m; ++i) q.g[i] = 0.0;
    q.hn[0] = beta;
}

// first stage of T <= GMRES_TILE sums V_t . w: reduce_stage1<RED_DOT>'s grid, body, tail and order per column, w loaded once
template <int T>
__global__ __launch_bounds__(RT) void gmres_dots_kernel(const double *__restrict__ V, int64_t ldv, const double *__restrict__ w,
                                                        int64_t n, const int64_t *__restrict__ state,
                                                        double *__restrict__ partial)
{
    if (state[1] != PCG_RUNNING) return;
    const int64_t n2 = n / 2, ld2 = ldv / 2;
    const double2 *V2 = reinterpret_cast<const double2 *>(V);
    const double2 *w2 = reinterpret_cast<const double2 *>(w);
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 wv = w2[i];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const double2 vv = V2[(int64_t)t * ld2 + i];
            acc[t] = acc[t] + vv.x * wv.x;
            acc[t] = acc[t] + vv.y * wv.y;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double wj = w[n - 1];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = acc[t] + V[(int64_t)t * ldv + n - 1] * wj;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t) __syncthreads();                                  // block_reduce's LDS slots are reused
        const double r = block_reduce<RED_SUM>(acc[t]);
        if (threadIdx.x == 0) partial[(int64_t)t * MAX_PARTIALS + blockIdx.x] = r;
    }
}

// second stage: workgroup i sums the partials of column i in index order (reduce_stage2<RED_SUM>'s order)
__global__ __launch_bounds__(RT) void gmres_dots_stage2_kernel(const double *__restrict__ partial, int np,
                                                               const int64_t *__restrict__ state, double *__restrict__ h_out)
{
    if (state[1] != PCG_RUNNING) return;
    const double *p = partial + (int64_t)blockIdx.x * MAX_PARTIALS;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) acc = acc + p[i];
    const double r = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) h_out[blockIdx.x] = r;
}

// the running subtraction over all c columns in one pass; SUMSQ also emits the partials of w.w (of the final w)
template <bool SUMSQ>
__global__ __launch_bounds__(RT) void gmres_update_kernel(const double *__restrict__ V, int64_t ldv, int c,
                                                          const double *__restrict__ h, double *__restrict__ w, int64_t n,
                                                          const int64_t *__restrict__ state, double *__restrict__ partial)
{
    if (state[1] != PCG_RUNNING) return;
    const int64_t n2 = n / 2, ld2 = ldv / 2;
    const double2 *V2 = reinterpret_cast<const double2 *>(V);
    double2 *w2 = reinterpret_cast<double2 *>(w);
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        double2 wv = w2[i];
#pragma unroll 4
        for (int t = 0; t < c; ++t) {
            const double ht = h[t];
            const double2 vv = V2[(int64_t)t * ld2 + i];
            wv.x = wv.x - ht * vv.x;
            wv.y = wv.y - ht * vv.y;
        }
        w2[i] = wv;
        if (SUMSQ) {
            acc = acc + wv.x * wv.x;
            acc = acc + wv.y * wv.y;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        double wj = w[n - 1];
        for (int t = 0; t < c; ++t) wj = wj - h[t] * V[(int64_t)t * ldv + n - 1];
        w[n - 1] = wj;
        if (SUMSQ) acc = acc + wj * wj;
    }
    if (SUMSQ) {
        const double r = block_reduce<RED_SUM>(acc);
        if (threadIdx.x == 0) partial[blockIdx.x] = r;
    }
}

// second stage of w.w, one workgroup; runs the small step where no all-reduce follows (gate != 0)
__global__ __launch_bounds__(RT) void gmres_update_stage2_kernel(const double *__restrict__ partial, int np, GmresSmall q, int j,
                                                                 int m, double *__restrict__ hist_k, int64_t iter, int gate,
                                                                 int64_t *__restrict__ state)
{
    if (state[1] != PCG_RUNNING) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) acc = acc + partial[i];
    const double nn = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) {
        q.nn[0] = nn;
        if (gate) gmres_small_step(q, j, m, nn, hist_k, iter, state);
    }
}

__global__ void gmres_small_step_kernel(GmresSmall q, int j, int m, double *__restrict__ hist_k, int64_t iter,
                                        int64_t *__restrict__ state)
{
    if (threadIdx.x == 0 && state[1] == PCG_RUNNING) gmres_small_step(q, j, m, q.nn[0], hist_k, iter, state);
}

// V_{j+1} = w / col_c: a division, not a multiplication by the reciprocal
template <bool PRECOND>
__global__ __launch_bounds__(256) void gmres_next_kernel(const double *__restrict__ w, const double *__restrict__ hn,
                                                         const double *__restrict__ dinv, double *__restrict__ v,
                                                         double *__restrict__ z, int64_t n, const int64_t *__restrict__ state)
{
    if (state[1] != PCG_RUNNING) return;
    const double d = hn[0];
    const int64_t n2 = n / 2;
    const double2 *w2 = reinterpret_cast<const double2 *>(w);
    const double2 *d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *v2 = reinterpret_cast<double2 *>(v);
    double2 *z2 = reinterpret_cast<double2 *>(z);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n2; i += stride) {
        const double2 wv = w2[i];
        double2 vv;
        vv.x = wv.x / d;
        vv.y = wv.y / d;
        v2[i] = vv;
        if (PRECOND) {
            const double2 dv = d2[i];
            double2 zv;
            zv.x = dv.x * vv.x;
            zv.y = dv.y * vv.y;
            z2[i] = zv;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t l = n - 1;
        const double vl = w[l] / d;
        v[l] = vl;
        if (PRECOND) z[l] = dinv[l] * vl;
    }
}

// cycle end: x = x + u or x + dinv .* u with u = y[0] V_0, u = u + y[i] V_i ascending.  state == NULL: the host's ungated finish
template <bool NTX, bool PRECOND>
__global__ __launch_bounds__(256) void gmres_xupdate_kernel(const double *__restrict__ V, int64_t ldv, int c,
                                                            const double *__restrict__ y, const double *__restrict__ dinv,
                                                            double *__restrict__ x, int64_t n, const int64_t *__restrict__ state)
{
    if (state && state[1] != PCG_RUNNING) return;
    const int64_t n2 = n / 2, ld2 = ldv / 2;
    const double2 *V2 = reinterpret_cast<const double2 *>(V);
    const double2 *d2 = reinterpret_cast<const double2 *>(dinv);
    double2 *x2 = reinterpret_cast<double2 *>(x);
    const double y0 = y[0];
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n2; i += stride) {
        double2 u = V2[i];
        u.x = y0 * u.x;
        u.y = y0 * u.y;
#pragma unroll 4
        for (int t = 1; t < c; ++t) {
            const double yt = y[t];
            const double2 vv = V2[(int64_t)t * ld2 + i];
            u.x = u.x + yt * vv.x;
            u.y = u.y + yt * vv.y;
        }
        if (PRECOND) {
            const double2 dv = d2[i];
            u.x = dv.x * u.x;
            u.y = dv.y * u.y;
        }
        double2 xv = NTX ? nt_load2(x2 + i) : x2[i];
        xv.x = xv.x + u.x;
        xv.y = xv.y + u.y;
        if (NTX) nt_store2(xv, x2 + i); else x2[i] = xv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t l = n - 1;
        double u = y0 * V[l];
        for (int t = 1; t < c; ++t) u = u + y[t] * V[(int64_t)t * ldv + l];
        if (PRECOND) u = dinv[l] * u;
        x[l] = x[l] + u;
    }
}

// restart: w = b - w (w holds A x), partials of w.w
__global__ __launch_bounds__(RT) void gmres_residual_kernel(const double *__restrict__ b, double *__restrict__ w, int64_t n,
                                                            const int64_t *__restrict__ state, double *__restrict__ partial)
{
    if (state[1] != PCG_RUNNING) return;
    const int64_t n2 = n / 2;
    const double2 *b2 = reinterpret_cast<const double2 *>(b);
    double2 *w2 = reinterpret_cast<double2 *>(w);
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * RT + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * RT;
    for (; i < n2; i += stride) {
        const double2 bv = b2[i];
        double2 wv = w2[i];
        wv.x = bv.x - wv.x;
        wv.y = bv.y - wv.y;
        w2[i] = wv;
        acc = acc + wv.x * wv.x;
        acc = acc + wv.y * wv.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double wj = b[n - 1] - w[n - 1];
        w[n - 1] = wj;
        acc = acc + wj * wj;
    }
    const double r = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// second stage of the restart's w.w, one workgroup; gate R and the new cycle's g where no all-reduce follows (gate != 0)
__global__ __launch_bounds__(RT) void gmres_residual_stage2_kernel(const double *__restrict__ partial, int np, GmresSmall q, int m,
                                                                   double *__restrict__ hist_k, int64_t iter, int gate,
                                                                   int64_t *__restrict__ state)
{
    if (state[1] != PCG_RUNNING) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) acc = acc + partial[i];
    const double rr = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) {
        q.nn[0] = rr;
        if (gate) gmres_restart_gate(q, m, rr, hist_k, iter, state);
    }
}

__global__ void gmres_restart_gate_kernel(GmresSmall q, int m, double *__restrict__ hist_k, int64_t iter,
                                          int64_t *__restrict__ state)
{
    if (threadIdx.x == 0 && state[1] == PCG_RUNNING) gmres_restart_gate(q, m, q.nn[0], hist_k, iter, state);
}

// y = R^-1 g over c columns by back substitution, one thread.  state == NULL: the host's ungated finish
__global__ void gmres_solve_kernel(GmresSmall q, int c, int m, const int64_t *__restrict__ state)
{
    if (threadIdx.x != 0 || (state && state[1] != PCG_RUNNING)) return;
    for (int i = c - 1; i >= 0; --i) {
        double t = q.g[i];
        for (int l = i + 1; l < c; ++l) t = t - q.R[(int64_t)l * m + i] * q.y[l];
        q.y[i] = t / q.R[(int64_t)i * m + i];
    }
}

// MODE 0: y = y + a*x   MODE 1: y = x + a*y   MODE 2: y = a*x   MODE 3: y = x / a
template <int MODE>
__global__ __launch_bounds__(256) void update_kernel(double alpha, const double *__restrict__ num,
                                                     const double *__restrict__ den,
                                                     const double *__restrict__ x,
                                                     double *__restrict__ y, int64_t n)
{
    const double a = dev_scalar(alpha, num, den);
    const int64_t n2 = n / 2;
    const double2 *x2 = reinterpret_cast<const double2 *>(x);
    double2 *y2 = reinterpret_cast<double2 *>(y);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n2; i += stride) {
        const double2 xv = x2[i];
        double2 yv;
        if (MODE == 0) { yv = y2[i]; yv.x = yv.x + a * xv.x; yv.y = yv.y + a * xv.y; }
        if (MODE == 1) { yv = y2[i]; yv.x = xv.x + a * yv.x; yv.y = xv.y + a * yv.y; }
        if (MODE == 2) { yv.x = a * xv.x; yv.y = a * xv.y; }
        if (MODE == 3) { yv.x = xv.x / a; yv.y = xv.y / a; }
        y2[i] = yv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t j = n - 1;
        if (MODE == 0) y[j] = y[j] + a * x[j];
        if (MODE == 1) y[j] = x[j] + a * y[j];
        if (MODE == 2) y[j] = a * x[j];
        if (MODE == 3) y[j] = x[j] / a;
    }
}

__global__ __launch_bounds__(256) void axpby_kernel(double a, const double *__restrict__ x,
                                                    double b, const double *__restrict__ y,
                                                    double *__restrict__ z, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n; i += stride) z[i] = a * x[i] + b * y[i];
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void fill_uniform_kernel(double *__restrict__ v, int64_t start,
                                                           int64_t count, uint64_t seed)
{
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < count; i += stride) {
        const uint64_t z = splitmix64(seed + 0x9E3779B97F4A7C15ULL * (uint64_t)(start + i + 1));
        v[i] = (double)(z >> 11) * 0x1.0p-53;
    }
}

static inline uint32_t ew_grid(int64_t n_items)
{
    int64_t g = (n_items + 255) / 256;
    if (g < 1) g = 1;
    if (g > 4096) g = 4096;
    return (uint32_t)g;
}

template <int MODE>
static int update_impl(double alpha, const double *num, const double *den, const double *x,
                       double *y, int64_t n, void *stream)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "update: negative size");
    if (n == 0) return HPCLA_OK;
    if (!x || !y) return set_error(HPCLA_ERR_INVALID, "update: null pointer");
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(y) & 15))
        return set_error(HPCLA_ERR_INVALID, "update: inputs must be 16-byte aligned");
    update_kernel<MODE><<<ew_grid(n / 2), 256, 0, as_stream(stream)>>>(alpha, num, den, x, y, n);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int64_t hpcla_reduce_work_bytes(void) { return (int64_t)MAX_PARTIALS * sizeof(double); }

HPCLA_API int hpcla_dot_f64(hpcla_comm_t *comm, const double *x, const double *y, int64_t n,
                            double *out_dev, void *work, void *stream)
{
    return reduce_impl<RED_DOT>(comm, x, y, n, out_dev, work, stream);
}
HPCLA_API int hpcla_nrm2sq_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev,
                               void *work, void *stream)
{
    return reduce_impl<RED_SQ>(comm, x, nullptr, n, out_dev, work, stream);
}
HPCLA_API int hpcla_asum_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev,
                             void *work, void *stream)
{
    return reduce_impl<RED_ABS>(comm, x, nullptr, n, out_dev, work, stream);
}
HPCLA_API int hpcla_amax_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev,
                             void *work, void *stream)
{
    return reduce_impl<RED_MAX>(comm, x, nullptr, n, out_dev, work, stream);
}

// maximum(v) / minimum(v) (src/vectors.jl:815-836).  minimum = -max(-x): the kernel negates on load and the
// caller negates the all-reduced result (out holds max(-x) when negate == 1).
HPCLA_API int hpcla_maxval_f64(hpcla_comm_t *comm, const double *x, int64_t n, int negate, double *out_dev,
                               void *work, void *stream)
{
    return reduce_impl<RED_MAXV>(comm, x, nullptr, n, out_dev, work, stream, negate ? 1.0 : 0.0);
}

HPCLA_API int hpcla_sum_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev, void *work,
                            void *stream)
{
    return reduce_impl<RED_SUM>(comm, x, nullptr, n, out_dev, work, stream);
}

// prod(v) (src/vectors.jl:853-858; an empty local part contributes one(T))
HPCLA_API int hpcla_prod_f64(hpcla_comm_t *comm, const double *x, int64_t n, double *out_dev, void *work,
                             void *stream)
{
    return reduce_impl<RED_PROD>(comm, x, nullptr, n, out_dev, work, stream);
}

HPCLA_API int hpcla_powsum_f64(hpcla_comm_t *comm, const double *x, int64_t n, double p, double *out_dev,
                               void *work, void *stream)
{
    if (!(p > 0.0)) return set_error(HPCLA_ERR_INVALID, "powsum: p must be positive");
    return reduce_impl<RED_POW>(comm, x, nullptr, n, out_dev, work, stream, p);
}

HPCLA_API int hpcla_axpy_f64(double alpha_host, const double *num_dev, const double *den_dev,
                             const double *x, double *y, int64_t n, void *stream)
{
    return update_impl<0>(alpha_host, num_dev, den_dev, x, y, n, stream);
}
HPCLA_API int hpcla_xpay_f64(const double *x, double alpha_host, const double *num_dev,
                             const double *den_dev, double *y, int64_t n, void *stream)
{
    return update_impl<1>(alpha_host, num_dev, den_dev, x, y, n, stream);
}
HPCLA_API int hpcla_scale_f64(double alpha_host, const double *x, double *y, int64_t n,
                              void *stream)
{
    return update_impl<2>(alpha_host, nullptr, nullptr, x, y, n, stream);
}
HPCLA_API int hpcla_divide_f64(const double *x, double a_host, double *y, int64_t n, void *stream)
{
    return update_impl<3>(a_host, nullptr, nullptr, x, y, n, stream);
}
HPCLA_API int hpcla_axpby_f64(double a, const double *x, double b, const double *y, double *z,
                              int64_t n, void *stream)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "axpby: negative size");
    if (n == 0) return HPCLA_OK;
    if (!x || !y || !z) return set_error(HPCLA_ERR_INVALID, "axpby: null pointer");
    axpby_kernel<<<ew_grid(n), 256, 0, as_stream(stream)>>>(a, x, b, y, z, n);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_cg_update_f64(hpcla_comm_t *comm, double alpha_host, const double *num_dev,
                                  const double *den_dev, const double *p, const double *Ap, double *x,
                                  double *r, int64_t n, double *rr_out_dev, void *work, void *stream)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "cg_update: negative size");
    if (!rr_out_dev || !work) return set_error(HPCLA_ERR_INVALID, "cg_update: null out/work");
    if (n > 0 && (!p || !Ap || !x || !r)) return set_error(HPCLA_ERR_INVALID, "cg_update: null vector");
    if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(Ap) | reinterpret_cast<uintptr_t>(x) |
         reinterpret_cast<uintptr_t>(r)) & 15)
        return set_error(HPCLA_ERR_INVALID, "cg_update: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    cg_update_kernel<<<g, RT, 0, as_stream(stream)>>>(alpha_host, num_dev, den_dev, p, Ap, x, r, n, partial);
    HPCLA_CHECK_LAUNCH();
    reduce_stage2<RED_SUM><<<1, RT, 0, as_stream(stream)>>>(partial, g, rr_out_dev);
    HPCLA_CHECK_LAUNCH();
    if (comm) return allreduce_on(comm, rr_out_dev, 1, 0, stream);
    return HPCLA_OK;
}

static int cg_nt_mask()
{
    static const int m = [] {
        const char *e = getenv("HPCLA_CG_NT");
        return e ? atoi(e) : 7;
    }();
    return m;
}

HPCLA_API int hpcla_cg_residual_f64(hpcla_comm_t *comm, double alpha_host, const double *num_dev,
                                    const double *den_dev, const double *Ap, double *r, int64_t n,
                                    double *rr_out_dev, void *work, void *stream)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "cg_residual: negative size");
    if (!rr_out_dev || !work) return set_error(HPCLA_ERR_INVALID, "cg_residual: null out/work");
    if (n > 0 && (!Ap || !r)) return set_error(HPCLA_ERR_INVALID, "cg_residual: null vector");
    if ((reinterpret_cast<uintptr_t>(Ap) | reinterpret_cast<uintptr_t>(r)) & 15)
        return set_error(HPCLA_ERR_INVALID, "cg_residual: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    if (cg_nt_mask() & 4)
        cg_residual_kernel<true><<<g, RT, 0, as_stream(stream)>>>(alpha_host, num_dev, den_dev, Ap, r, n, partial);
    else
        cg_residual_kernel<false><<<g, RT, 0, as_stream(stream)>>>(alpha_host, num_dev, den_dev, Ap, r, n, partial);
    HPCLA_CHECK_LAUNCH();
    reduce_stage2<RED_SUM><<<1, RT, 0, as_stream(stream)>>>(partial, g, rr_out_dev);
    HPCLA_CHECK_LAUNCH();
    if (comm) return allreduce_on(comm, rr_out_dev, 1, 0, stream);
    return HPCLA_OK;
}

HPCLA_API int hpcla_cg_direction_f64(double alpha_host, const double *a_num_dev, const double *a_den_dev,
                                     double beta_host, const double *b_num_dev, const double *b_den_dev,
                                     const double *r, double *x, double *p, int64_t n, void *stream)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "cg_direction: negative size");
    if (n == 0) return HPCLA_OK;
    if (!r || !x || !p) return set_error(HPCLA_ERR_INVALID, "cg_direction: null vector");
    if ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(p)) & 15)
        return set_error(HPCLA_ERR_INVALID, "cg_direction: vectors must be 16-byte aligned");
    const int m = cg_nt_mask();
#define HPCLA_CG_DIR(NX, NR)                                                                                           \
    cg_direction_kernel<NX, NR><<<ew_grid(n / 2), 256, 0, as_stream(stream)>>>(alpha_host, a_num_dev, a_den_dev, beta_host, \
                                                                               b_num_dev, b_den_dev, r, x, p, n)
    if ((m & 1) && (m & 2)) HPCLA_CG_DIR(true, true);
    else if (m & 1) HPCLA_CG_DIR(true, false);
    else if (m & 2) HPCLA_CG_DIR(false, true);
    else HPCLA_CG_DIR(false, false);
#undef HPCLA_CG_DIR
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// scratch of the gated pair: two arrays of stage-1 partials, then the solve's state (its last 32 bytes)
HPCLA_API int64_t hpcla_pcg_work_bytes(void)
{
    return (int64_t)(2 * MAX_PARTIALS + PCG_STATE_WORDS) * (int64_t)sizeof(double);
}

HPCLA_API int hpcla_pcg_residual_f64(hpcla_comm_t *comm, const double *num_dev, const double *den_dev, const double *Ap,
                                     const double *dinv, double *r, int64_t n, int64_t iter, int64_t *state_dev,
                                     double *pair_out_dev, void *work, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "pcg_residual: negative size or iteration < 1");
    if (!num_dev || !den_dev || !state_dev || !pair_out_dev || !work)
        return set_error(HPCLA_ERR_INVALID, "pcg_residual: null scalar / state / out / work");
    if (n > 0 && (!Ap || !r)) return set_error(HPCLA_ERR_INVALID, "pcg_residual: null vector");
    if ((reinterpret_cast<uintptr_t>(Ap) | reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(dinv)) & 15)
        return set_error(HPCLA_ERR_INVALID, "pcg_residual: vectors must be 16-byte aligned");
    double *partial_rr = reinterpret_cast<double *>(work), *partial_rz = partial_rr + MAX_PARTIALS;
    const int g = reduce_grid(n);
    hipStream_t s = as_stream(stream);
    const bool nt = (cg_nt_mask() & 4) != 0;
#define HPCLA_PCG_RES(NT, PC) \
    pcg_residual_kernel<NT, PC><<<g, RT, 0, s>>>(num_dev, den_dev, Ap, dinv, r, n, state_dev, partial_rr, partial_rz)
    if (dinv) { if (nt) HPCLA_PCG_RES(true, true); else HPCLA_PCG_RES(false, true); }
    else      { if (nt) HPCLA_PCG_RES(true, false); else HPCLA_PCG_RES(false, false); }
#undef HPCLA_PCG_RES
    HPCLA_CHECK_LAUNCH();
    const int gate_b = comm ? 0 : 1;
    if (dinv) pcg_stage2_kernel<true><<<1, RT, 0, s>>>(partial_rr, partial_rz, g, den_dev, iter, gate_b, state_dev, pair_out_dev);
    else pcg_stage2_kernel<false><<<1, RT, 0, s>>>(partial_rr, partial_rz, g, den_dev, iter, gate_b, state_dev, pair_out_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, pair_out_dev, 2, 0, stream);   // rr and rz travel as ONE pair
    if (rc) return rc;
    pcg_gate_b_kernel<<<1, 64, 0, s>>>(pair_out_dev, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_pcg_direction_f64(const double *a_num_dev, const double *a_den_dev, const double *b_num_dev,
                                      const double *b_den_dev, const double *r, const double *dinv, double *x, double *p,
                                      int64_t n, int64_t iter, const int64_t *state_dev, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "pcg_direction: negative size or iteration < 1");
    if (!a_num_dev || !a_den_dev || !b_num_dev || !b_den_dev || !state_dev)
        return set_error(HPCLA_ERR_INVALID, "pcg_direction: null scalar / state");
    if (n == 0) return HPCLA_OK;
    if (!r || !x || !p) return set_error(HPCLA_ERR_INVALID, "pcg_direction: null vector");
    if ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(p) |
         reinterpret_cast<uintptr_t>(dinv)) & 15)
        return set_error(HPCLA_ERR_INVALID, "pcg_direction: vectors must be 16-byte aligned");
    const int m = cg_nt_mask();
#define HPCLA_PCG_DIR(NX, NR)                                                                                          \
    do {                                                                                                               \
        if (dinv)                                                                                                      \
            pcg_direction_kernel<NX, NR, true><<<ew_grid(n / 2), 256, 0, as_stream(stream)>>>(                         \
                a_num_dev, a_den_dev, b_num_dev, b_den_dev, r, dinv, x, p, n, iter, state_dev);                        \
        else                                                                                                           \
            pcg_direction_kernel<NX, NR, false><<<ew_grid(n / 2), 256, 0, as_stream(stream)>>>(                        \
                a_num_dev, a_den_dev, b_num_dev, b_den_dev, r, dinv, x, p, n, iter, state_dev);                        \
    } while (0)
    if ((m & 1) && (m & 2)) HPCLA_PCG_DIR(true, true);
    else if (m & 1) HPCLA_PCG_DIR(true, false);
    else if (m & 2) HPCLA_PCG_DIR(false, true);
    else HPCLA_PCG_DIR(false, false);
#undef HPCLA_PCG_DIR
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// scratch of the gated BiCGStab steps: three arrays of stage-1 partials, then the solve's state (its last 32 bytes)
HPCLA_API int64_t hpcla_bicgstab_work_bytes(void)
{
    return (int64_t)(BICG_PARTIAL_ARRAYS * MAX_PARTIALS + PCG_STATE_WORDS) * (int64_t)sizeof(double);
}

HPCLA_API int hpcla_bicg_dot_f64(hpcla_comm_t *comm, const double *rhat, const double *v, int64_t n, int64_t iter,
                                 const double *rho_dev, int64_t *state_dev, double *rv_out_dev, void *work, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "bicg_dot: negative size or iteration < 1");
    if (!rho_dev || !state_dev || !rv_out_dev || !work)
        return set_error(HPCLA_ERR_INVALID, "bicg_dot: null scalar / state / out / work");
    if (n > 0 && (!rhat || !v)) return set_error(HPCLA_ERR_INVALID, "bicg_dot: null vector");
    if (misaligned16({rhat, v})) return set_error(HPCLA_ERR_INVALID, "bicg_dot: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    hipStream_t s = as_stream(stream);
    bicg_dot_kernel<<<g, RT, 0, s>>>(rhat, v, n, state_dev, partial);
    HPCLA_CHECK_LAUNCH();
    bicg_dot_stage2_kernel<<<1, RT, 0, s>>>(partial, g, rho_dev, iter, comm ? 0 : 1, state_dev, rv_out_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, rv_out_dev, 1, 0, stream);
    if (rc) return rc;
    bicg_gate_a_kernel<<<1, 64, 0, s>>>(rho_dev, rv_out_dev, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_bicg_s_f64(const double *rho_dev, const double *rv_dev, const double *r, const double *v,
                               const double *dinv, double *s, double *sh, int64_t n, int64_t iter, const int64_t *state_dev,
                               void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "bicg_s: negative size or iteration < 1");
    if (!rho_dev || !rv_dev || !state_dev) return set_error(HPCLA_ERR_INVALID, "bicg_s: null scalar / state");
    if (n == 0) return HPCLA_OK;
    if (!r || !v || !s || (dinv && !sh)) return set_error(HPCLA_ERR_INVALID, "bicg_s: null vector");
    if (misaligned16({r, v, dinv, s, dinv ? sh : nullptr}))
        return set_error(HPCLA_ERR_INVALID, "bicg_s: vectors must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    if (dinv) bicg_s_kernel<true><<<ew_grid(n / 2), 256, 0, st>>>(rho_dev, rv_dev, r, v, dinv, s, sh, n, state_dev);
    else bicg_s_kernel<false><<<ew_grid(n / 2), 256, 0, st>>>(rho_dev, rv_dev, r, v, nullptr, s, nullptr, n, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_bicg_tts_f64(hpcla_comm_t *comm, const double *t, const double *s, int64_t n, int64_t iter,
                                 int64_t *state_dev, double *triple_out_dev, void *work, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "bicg_tts: negative size or iteration < 1");
    if (!state_dev || !triple_out_dev || !work) return set_error(HPCLA_ERR_INVALID, "bicg_tts: null state / out / work");
    if (n > 0 && (!t || !s)) return set_error(HPCLA_ERR_INVALID, "bicg_tts: null vector");
    if (misaligned16({t, s})) return set_error(HPCLA_ERR_INVALID, "bicg_tts: vectors must be 16-byte aligned");
    double *p_ts = reinterpret_cast<double *>(work), *p_tt = p_ts + MAX_PARTIALS, *p_ss = p_tt + MAX_PARTIALS;
    const int g = reduce_grid(n);
    hipStream_t st = as_stream(stream);
    bicg_tts_kernel<<<g, RT, 0, st>>>(t, s, n, state_dev, p_ts, p_tt, p_ss);
    HPCLA_CHECK_LAUNCH();
    bicg_tts_stage2_kernel<<<1, RT, 0, st>>>(p_ts, p_tt, p_ss, g, iter, comm ? 0 : 1, state_dev, triple_out_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, triple_out_dev, 3, 0, stream);   // ts, tt and ss travel as ONE triple
    if (rc) return rc;
    bicg_gate_st_kernel<<<1, 64, 0, st>>>(triple_out_dev, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_bicg_xr_f64(hpcla_comm_t *comm, const double *rho_dev, const double *rv_dev, const double *triple_dev,
                                const double *ph, const double *sh, const double *s, const double *t, const double *rhat,
                                double *x, double *r, int64_t n, int64_t iter, int64_t *state_dev, double *pair_out_dev,
                                void *work, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "bicg_xr: negative size or iteration < 1");
    if (!rho_dev || !rv_dev || !triple_dev || !state_dev || !pair_out_dev || !work)
        return set_error(HPCLA_ERR_INVALID, "bicg_xr: null scalar / state / out / work");
    if (n > 0 && (!ph || !s || !t || !rhat || !x || !r)) return set_error(HPCLA_ERR_INVALID, "bicg_xr: null vector");
    if (misaligned16({ph, sh, s, t, rhat, x, r}))
        return set_error(HPCLA_ERR_INVALID, "bicg_xr: vectors must be 16-byte aligned");
    double *p_rr = reinterpret_cast<double *>(work), *p_rho = p_rr + MAX_PARTIALS;
    const int g = reduce_grid(n);
    hipStream_t st = as_stream(stream);
    const int m = cg_nt_mask();
#define HPCLA_BICG_XR(NX, NT)                                                                                          \
    do {                                                                                                               \
        if (sh)                                                                                                        \
            bicg_xr_kernel<NX, NT, true><<<g, RT, 0, st>>>(rho_dev, rv_dev, triple_dev, triple_dev + 1, ph, sh, s, t, rhat, x, \
                                                           r, n, iter, state_dev, p_rr, p_rho);                        \
        else                                                                                                           \
            bicg_xr_kernel<NX, NT, false><<<g, RT, 0, st>>>(rho_dev, rv_dev, triple_dev, triple_dev + 1, ph, nullptr, s, t,  \
                                                            rhat, x, r, n, iter, state_dev, p_rr, p_rho);              \
    } while (0)
    if ((m & 1) && (m & 4)) HPCLA_BICG_XR(true, true);
    else if (m & 1) HPCLA_BICG_XR(true, false);
    else if (m & 4) HPCLA_BICG_XR(false, true);
    else HPCLA_BICG_XR(false, false);
#undef HPCLA_BICG_XR
    HPCLA_CHECK_LAUNCH();
    bicg_xr_stage2_kernel<<<1, RT, 0, st>>>(p_rr, p_rho, g, triple_dev, iter, comm ? 0 : 1, state_dev, pair_out_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, pair_out_dev, 2, 0, stream);     // rr and rho' travel as ONE pair
    if (rc) return rc;
    bicg_gate_bo_kernel<<<1, 64, 0, st>>>(pair_out_dev, triple_dev, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_bicg_p_f64(const double *rho_new_dev, const double *rho_dev, const double *rv_dev,
                               const double *triple_dev, const double *r, const double *v, const double *dinv, double *p,
                               double *ph, int64_t n, int64_t iter, const int64_t *state_dev, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "bicg_p: negative size or iteration < 1");
    if (!rho_new_dev || !rho_dev || !rv_dev || !triple_dev || !state_dev)
        return set_error(HPCLA_ERR_INVALID, "bicg_p: null scalar / state");
    if (n == 0) return HPCLA_OK;
    if (!r || !v || !p || (dinv && !ph)) return set_error(HPCLA_ERR_INVALID, "bicg_p: null vector");
    if (misaligned16({r, v, dinv, p, dinv ? ph : nullptr}))
        return set_error(HPCLA_ERR_INVALID, "bicg_p: vectors must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    if (dinv)
        bicg_p_kernel<true><<<ew_grid(n / 2), 256, 0, st>>>(rho_new_dev, rho_dev, rv_dev, triple_dev, triple_dev + 1, r, v, dinv,
                                                            p, ph, n, state_dev);
    else
        bicg_p_kernel<false><<<ew_grid(n / 2), 256, 0, st>>>(rho_new_dev, rho_dev, rv_dev, triple_dev, triple_dev + 1, r, v,
                                                             nullptr, p, nullptr, n, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// scratch of the gated LSQR steps: one array of stage-1 partials, then the solve's state (its last 32 bytes)
HPCLA_API int64_t hpcla_lsqr_work_bytes(void)
{
    return (int64_t)(MAX_PARTIALS + PCG_STATE_WORDS) * (int64_t)sizeof(double);
}

HPCLA_API int hpcla_lsqr_u_f64(hpcla_comm_t *comm, double *scal_dev, const double *tu, double *uh, int64_t n, int64_t iter,
                               const int64_t *state_dev, void *work, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "lsqr_u: negative size or iteration < 1");
    if (!scal_dev || !state_dev || !work) return set_error(HPCLA_ERR_INVALID, "lsqr_u: null scalars / state / work");
    if (n > 0 && (!tu || !uh)) return set_error(HPCLA_ERR_INVALID, "lsqr_u: null vector");
    if (misaligned16({tu, uh})) return set_error(HPCLA_ERR_INVALID, "lsqr_u: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    hipStream_t s = as_stream(stream);
    if (cg_nt_mask() & 4) lsqr_u_kernel<true><<<g, RT, 0, s>>>(scal_dev, tu, uh, n, state_dev, partial);
    else lsqr_u_kernel<false><<<g, RT, 0, s>>>(scal_dev, tu, uh, n, state_dev, partial);
    HPCLA_CHECK_LAUNCH();
    lsqr_u_stage2_kernel<<<1, RT, 0, s>>>(partial, g, state_dev, scal_dev);
    HPCLA_CHECK_LAUNCH();
    if (comm) return allreduce_on(comm, scal_dev + LSQR_UU, 1, 0, stream);
    return HPCLA_OK;
}

HPCLA_API int hpcla_lsqr_v_f64(hpcla_comm_t *comm, double *scal_dev, const double *tv, double *vh, int64_t n, int64_t iter,
                               int64_t *state_dev, double *pair_out_dev, void *work, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "lsqr_v: negative size or iteration < 1");
    if (!scal_dev || !state_dev || !work) return set_error(HPCLA_ERR_INVALID, "lsqr_v: null scalars / state / work");
    if (n > 0 && (!tv || !vh)) return set_error(HPCLA_ERR_INVALID, "lsqr_v: null vector");
    if (misaligned16({tv, vh})) return set_error(HPCLA_ERR_INVALID, "lsqr_v: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    hipStream_t s = as_stream(stream);
    if (cg_nt_mask() & 4) lsqr_v_kernel<true><<<g, RT, 0, s>>>(scal_dev, tv, vh, n, state_dev, partial);
    else lsqr_v_kernel<false><<<g, RT, 0, s>>>(scal_dev, tv, vh, n, state_dev, partial);
    HPCLA_CHECK_LAUNCH();
    lsqr_v_stage2_kernel<<<1, RT, 0, s>>>(partial, g, iter, state_dev, scal_dev, comm ? nullptr : pair_out_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, scal_dev + LSQR_VV, 1, 0, stream);
    if (rc) return rc;
    if (!pair_out_dev) return HPCLA_OK;
    lsqr_step_kernel<<<1, 64, 0, s>>>(scal_dev, pair_out_dev, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_lsqr_xw_f64(const double *scal_dev, const double *vh, double *x, double *w, int64_t n, int64_t iter,
                                const int64_t *state_dev, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "lsqr_xw: negative size or iteration < 1");
    if (!scal_dev || !state_dev) return set_error(HPCLA_ERR_INVALID, "lsqr_xw: null scalars / state");
    if (n == 0) return HPCLA_OK;
    if (!vh || !x || !w) return set_error(HPCLA_ERR_INVALID, "lsqr_xw: null vector");
    if (misaligned16({vh, x, w})) return set_error(HPCLA_ERR_INVALID, "lsqr_xw: vectors must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    if (cg_nt_mask() & 1) lsqr_xw_kernel<true><<<ew_grid(n / 2), 256, 0, s>>>(scal_dev, vh, x, w, n, iter, state_dev);
    else lsqr_xw_kernel<false><<<ew_grid(n / 2), 256, 0, s>>>(scal_dev, vh, x, w, n, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// scratch of the gated MINRES steps: one array of stage-1 partials, then the solve's state (its last 32 bytes)
HPCLA_API int64_t hpcla_minres_work_bytes(void)
{
    return (int64_t)(MAX_PARTIALS + PCG_STATE_WORDS) * (int64_t)sizeof(double);
}

HPCLA_API int hpcla_minres_r_f64(hpcla_comm_t *comm, double *scal_dev, const double *t, const double *r2, const double *dinv,
                                 double *r1, double *yn, int64_t n, int64_t iter, int64_t *state_dev, double *pair_out_dev,
                                 void *work, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "minres_r: negative size or iteration < 1");
    if (!scal_dev || !state_dev || !work) return set_error(HPCLA_ERR_INVALID, "minres_r: null scalars / state / work");
    if (n > 0 && (!t || !r2 || !r1 || (dinv && !yn))) return set_error(HPCLA_ERR_INVALID, "minres_r: null vector");
    if (n > 0 && (r1 == r2 || r1 == t || (dinv && (yn == r1 || yn == r2 || yn == t))))
        return set_error(HPCLA_ERR_INVALID, "minres_r: the written vectors must not alias the others");
    if (misaligned16({t, r2, dinv, r1, dinv ? yn : nullptr}))
        return set_error(HPCLA_ERR_INVALID, "minres_r: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    hipStream_t s = as_stream(stream);
    const bool nt = cg_nt_mask() & 4;
#define HPCLA_MINRES_R(NT, PC) minres_r_kernel<NT, PC><<<g, RT, 0, s>>>(scal_dev, t, r2, dinv, r1, yn, n, iter, state_dev, partial)
    if (dinv) {
        if (nt) HPCLA_MINRES_R(true, true); else HPCLA_MINRES_R(false, true);
    } else {
        if (nt) HPCLA_MINRES_R(true, false); else HPCLA_MINRES_R(false, false);
    }
#undef HPCLA_MINRES_R
    HPCLA_CHECK_LAUNCH();
    minres_r_stage2_kernel<<<1, RT, 0, s>>>(partial, g, iter, state_dev, scal_dev, comm ? nullptr : pair_out_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, scal_dev + MINRES_BB, 1, 0, stream);
    if (rc) return rc;
    if (!pair_out_dev) return HPCLA_OK;
    minres_step_kernel<<<1, 64, 0, s>>>(scal_dev, pair_out_dev, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_minres_xw_f64(const double *scal_dev, const double *y, const double *w2, double *w1, double *x, int64_t n,
                                  int64_t iter, const int64_t *state_dev, void *stream)
{
    if (n < 0 || iter < 1) return set_error(HPCLA_ERR_INVALID, "minres_xw: negative size or iteration < 1");
    if (!scal_dev || !state_dev) return set_error(HPCLA_ERR_INVALID, "minres_xw: null scalars / state");
    if (n == 0) return HPCLA_OK;
    if (!y || !w2 || !w1 || !x) return set_error(HPCLA_ERR_INVALID, "minres_xw: null vector");
    if (w1 == w2 || w1 == y || w1 == x || x == y || x == w2)
        return set_error(HPCLA_ERR_INVALID, "minres_xw: the written vectors must not alias the others");
    if (misaligned16({y, w2, w1, x})) return set_error(HPCLA_ERR_INVALID, "minres_xw: vectors must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    if (cg_nt_mask() & 1) minres_xw_kernel<true><<<ew_grid(n / 2), 256, 0, s>>>(scal_dev, y, w2, w1, x, n, iter, state_dev);
    else minres_xw_kernel<false><<<ew_grid(n / 2), 256, 0, s>>>(scal_dev, y, w2, w1, x, n, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// scratch of the gated GMRES steps: one array of stage-1 partials per column of the widest dots call (whole tiles), then the
// solve's state (its last 32 bytes)
HPCLA_API int64_t hpcla_gmres_work_bytes(int restart)
{
    if (restart < 1 || restart > GMRES_MAX_RESTART) return -1;
    const int64_t cols = (int64_t)((restart + GMRES_TILE - 1) / GMRES_TILE) * GMRES_TILE;
    return (cols * MAX_PARTIALS + PCG_STATE_WORDS) * (int64_t)sizeof(double);
}

// where the small arrays live in the solve's one buffer of doubles: which = 0 .. 9 for R, c, s, g, h1, h2, col, y, nn, hn;
// which = 10: the buffer's length
HPCLA_API int64_t hpcla_gmres_small_offset(int restart, int which)
{
    if (restart < 1 || restart > GMRES_MAX_RESTART || which < 0 || which > 10) return -1;
    int64_t off[11];
    gmres_small_offsets(restart, off);
    return off[which];
}

static inline bool gmres_bad_basis(int64_t n, int64_t ldv, int ncols, int restart)
{
    return n < 0 || ldv < n || (ldv & 1) || ncols < 1 || restart < 1 || restart > GMRES_MAX_RESTART || ncols > restart;
}

HPCLA_API int hpcla_gmres_dots_f64(hpcla_comm_t *comm, const double *V, int64_t ldv, int ncols, const double *w, int64_t n,
                                   const int64_t *state_dev, double *h_out_dev, void *work, void *stream)
{
    if (gmres_bad_basis(n, ldv, ncols, GMRES_MAX_RESTART))
        return set_error(HPCLA_ERR_INVALID, "gmres_dots: negative size, odd or short pitch, or column count outside 1..64");
    if (!state_dev || !h_out_dev || !work) return set_error(HPCLA_ERR_INVALID, "gmres_dots: null state / out / work");
    if (n > 0 && (!V || !w)) return set_error(HPCLA_ERR_INVALID, "gmres_dots: null vector");
    if (misaligned16({V, w})) return set_error(HPCLA_ERR_INVALID, "gmres_dots: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    hipStream_t s = as_stream(stream);
    for (int c0 = 0; c0 < ncols; c0 += GMRES_TILE) {
        const double *Vt = V + (int64_t)c0 * ldv;
        double *pt = partial + (int64_t)c0 * MAX_PARTIALS;
#define HPCLA_GMRES_DOTS(T) case T: gmres_dots_kernel<T><<<g, RT, 0, s>>>(Vt, ldv, w, n, state_dev, pt); break
        switch (ncols - c0 < GMRES_TILE ? ncols - c0 : GMRES_TILE) {
            HPCLA_GMRES_DOTS(1);
            HPCLA_GMRES_DOTS(2);
            HPCLA_GMRES_DOTS(3);
            HPCLA_GMRES_DOTS(4);
            HPCLA_GMRES_DOTS(5);
            HPCLA_GMRES_DOTS(6);
            HPCLA_GMRES_DOTS(7);
            HPCLA_GMRES_DOTS(8);
        }
#undef HPCLA_GMRES_DOTS
        HPCLA_CHECK_LAUNCH();
    }
    static_assert(GMRES_TILE == 8, "the switch above covers tiles of 1 .. 8 columns");
    gmres_dots_stage2_kernel<<<ncols, RT, 0, s>>>(partial, g, state_dev, h_out_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    for (int c0 = 0; c0 < ncols; c0 += AR_MAX) {                 // slices of AR_MAX: each takes the window path
        const int rc = allreduce_on(comm, h_out_dev + c0, ncols - c0 < AR_MAX ? ncols - c0 : AR_MAX, 0, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

// small_dev == NULL: the first pass, w only.  Else the second pass: also nn = w.w (one all-reduce), then the small step of
// column j = ncols - 1 from small's h1, h2 and nn, with gates D and C; hist_k_dev receives g[j+1]^2
HPCLA_API int hpcla_gmres_update_f64(hpcla_comm_t *comm, const double *V, int64_t ldv, int ncols, const double *h_dev, double *w,
                                     int64_t n, int64_t iter, int restart, double *small_dev, double *hist_k_dev,
                                     int64_t *state_dev, void *work, void *stream)
{
    if (gmres_bad_basis(n, ldv, ncols, small_dev ? restart : GMRES_MAX_RESTART) || iter < 1)
        return set_error(HPCLA_ERR_INVALID, "gmres_update: negative size, odd or short pitch, bad column count or iteration < 1");
    if (!h_dev || !state_dev || (small_dev && (!hist_k_dev || !work)))
        return set_error(HPCLA_ERR_INVALID, "gmres_update: null coefficients / state / history / work");
    if (n > 0 && (!V || !w)) return set_error(HPCLA_ERR_INVALID, "gmres_update: null vector");
    if (misaligned16({V, w})) return set_error(HPCLA_ERR_INVALID, "gmres_update: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    hipStream_t s = as_stream(stream);
    if (!small_dev) {
        gmres_update_kernel<false><<<g, RT, 0, s>>>(V, ldv, ncols, h_dev, w, n, state_dev, nullptr);
        HPCLA_CHECK_LAUNCH();
        return HPCLA_OK;
    }
    GmresSmall q;
    gmres_small_layout(restart, small_dev, &q);
    gmres_update_kernel<true><<<g, RT, 0, s>>>(V, ldv, ncols, h_dev, w, n, state_dev, partial);
    HPCLA_CHECK_LAUNCH();
    gmres_update_stage2_kernel<<<1, RT, 0, s>>>(partial, g, q, ncols - 1, restart, hist_k_dev, iter, comm ? 0 : 1, state_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, q.nn, 1, 0, stream);
    if (rc) return rc;
    gmres_small_step_kernel<<<1, 64, 0, s>>>(q, ncols - 1, restart, hist_k_dev, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_gmres_next_f64(const double *w, const double *hn_dev, const double *dinv, double *v_next, double *z,
                                   int64_t n, const int64_t *state_dev, void *stream)
{
    if (n < 0) return set_error(HPCLA_ERR_INVALID, "gmres_next: negative size");
    if (!hn_dev || !state_dev) return set_error(HPCLA_ERR_INVALID, "gmres_next: null scalar / state");
    if (n == 0) return HPCLA_OK;
    if (!w || !v_next || (dinv && !z)) return set_error(HPCLA_ERR_INVALID, "gmres_next: null vector");
    if (misaligned16({w, dinv, v_next, dinv ? z : nullptr}))
        return set_error(HPCLA_ERR_INVALID, "gmres_next: vectors must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    if (dinv) gmres_next_kernel<true><<<ew_grid(n / 2), 256, 0, s>>>(w, hn_dev, dinv, v_next, z, n, state_dev);
    else gmres_next_kernel<false><<<ew_grid(n / 2), 256, 0, s>>>(w, hn_dev, nullptr, v_next, nullptr, n, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// state_dev == NULL: ungated (the finish of an open cycle)
HPCLA_API int hpcla_gmres_solve_f64(int ncols, int restart, double *small_dev, const int64_t *state_dev, void *stream)
{
    if (restart < 1 || restart > GMRES_MAX_RESTART || ncols < 1 || ncols > restart)
        return set_error(HPCLA_ERR_INVALID, "gmres_solve: restart outside 1..64 or column count outside 1..restart");
    if (!small_dev) return set_error(HPCLA_ERR_INVALID, "gmres_solve: null small arrays");
    GmresSmall q;
    gmres_small_layout(restart, small_dev, &q);
    gmres_solve_kernel<<<1, 64, 0, as_stream(stream)>>>(q, ncols, restart, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_gmres_xupdate_f64(const double *V, int64_t ldv, int ncols, const double *y_dev, const double *dinv, double *x,
                                      int64_t n, const int64_t *state_dev, void *stream)
{
    if (gmres_bad_basis(n, ldv, ncols, GMRES_MAX_RESTART))
        return set_error(HPCLA_ERR_INVALID, "gmres_xupdate: negative size, odd or short pitch, or column count outside 1..64");
    if (!y_dev) return set_error(HPCLA_ERR_INVALID, "gmres_xupdate: null coefficients");
    if (n == 0) return HPCLA_OK;
    if (!V || !x) return set_error(HPCLA_ERR_INVALID, "gmres_xupdate: null vector");
    if (misaligned16({V, dinv, x})) return set_error(HPCLA_ERR_INVALID, "gmres_xupdate: vectors must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    const uint32_t g = ew_grid(n / 2);
#define HPCLA_GMRES_XUP(NX)                                                                                            \
    do {                                                                                                               \
        if (dinv) gmres_xupdate_kernel<NX, true><<<g, 256, 0, s>>>(V, ldv, ncols, y_dev, dinv, x, n, state_dev);       \
        else gmres_xupdate_kernel<NX, false><<<g, 256, 0, s>>>(V, ldv, ncols, y_dev, nullptr, x, n, state_dev);        \
    } while (0)
    if (cg_nt_mask() & 1) HPCLA_GMRES_XUP(true);
    else HPCLA_GMRES_XUP(false);
#undef HPCLA_GMRES_XUP
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// w = b - w with rr = w.w (one all-reduce), gate R at iteration iter >= 0, else the new cycle's g = (sqrt(rr), 0, ...), hn
HPCLA_API int hpcla_gmres_residual_f64(hpcla_comm_t *comm, const double *b, double *w, int64_t n, int64_t iter, int restart,
                                       double *small_dev, double *hist_k_dev, int64_t *state_dev, void *work, void *stream)
{
    if (n < 0 || iter < 0 || restart < 1 || restart > GMRES_MAX_RESTART)
        return set_error(HPCLA_ERR_INVALID, "gmres_residual: negative size or iteration, or restart outside 1..64");
    if (!small_dev || !hist_k_dev || !state_dev || !work)
        return set_error(HPCLA_ERR_INVALID, "gmres_residual: null small arrays / history / state / work");
    if (n > 0 && (!b || !w)) return set_error(HPCLA_ERR_INVALID, "gmres_residual: null vector");
    if (misaligned16({b, w})) return set_error(HPCLA_ERR_INVALID, "gmres_residual: vectors must be 16-byte aligned");
    GmresSmall q;
    gmres_small_layout(restart, small_dev, &q);
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    hipStream_t s = as_stream(stream);
    gmres_residual_kernel<<<g, RT, 0, s>>>(b, w, n, state_dev, partial);
    HPCLA_CHECK_LAUNCH();
    gmres_residual_stage2_kernel<<<1, RT, 0, s>>>(partial, g, q, restart, hist_k_dev, iter, comm ? 0 : 1, state_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, q.nn, 1, 0, stream);
    if (rc) return rc;
    gmres_restart_gate_kernel<<<1, 64, 0, s>>>(q, restart, hist_k_dev, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// the host's finish of an open cycle of ncols columns, ungated: y = R^-1 g, then x = x + K (V y)
HPCLA_API int hpcla_gmres_finish_f64(const double *V, int64_t ldv, int ncols, int restart, double *small_dev, const double *dinv,
                                     double *x, int64_t n, void *stream)
{
    if (ncols == 0) return HPCLA_OK;
    int rc = hpcla_gmres_solve_f64(ncols, restart, small_dev, nullptr, stream);
    if (rc) return rc;
    GmresSmall q;
    gmres_small_layout(restart, small_dev, &q);
    return hpcla_gmres_xupdate_f64(V, ldv, ncols, q.y, dinv, x, n, nullptr, stream);
}

// ---- the Lanczos step of hp.eigsh (thick-restart Lanczos, full CGS2 reorthogonalisation; hpcla_eigsh_steps_*) ---------------
// Column j of a cycle of m = ncv columns, c = j + 1 basis columns, iter 1-based over the whole solve: w = A V_j (ungated),
// gmres_dots, gmres_update (first pass), gmres_dots, then THIS second pass -- gmres_update_kernel<true> as it is, and the
// Lanczos small step in place of the Givens one.  It keeps the projected matrix: T (m x m, column j at T + j*m), beta (m):
//   N  nn != nn                         -> status 2 (breakdown), done_iter = iter - 1; nothing of column j is stored
//   T[i, j] = h1[i] + h2[i], i <= j;  beta[j] = hn = sqrt(nn)
//   I  nn == 0                          -> status 4 (invariant), done_iter = iter; column j is stored
// gmres_next then writes V_{j+1} = w / hn (gated: not behind a stop).  Bytes per row and launches are the GMRES step's.
constexpr int64_t EIGSH_INVARIANT = 4;

struct EigshSmall {
    double *T, *beta, *h1, *h2, *nn, *hn;                    // T: m x m;  beta, h1, h2: m;  nn, hn: 1
};

static void eigsh_small_offsets(int m, int64_t off[7])          // off[6]: the buffer's length
{
    const int64_t len[6] = {(int64_t)m * m, m, m, m, 1, 1};
    off[0] = 0;
    for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + len[i];
}

static void eigsh_small_layout(int m, double *base, EigshSmall *q)
{
    int64_t off[7];
    eigsh_small_offsets(m, off);
    *q = EigshSmall{base + off[0], base + off[1], base + off[2], base + off[3], base + off[4], base + off[5]};
}

__device__ void eigsh_small_step(const EigshSmall &q, int j, int m, double nn, int64_t iter, int64_t *state)
{
    if (nn != nn) {                                              // gate N
        state[0] = iter - 1;
        state[1] = PCG_BREAKDOWN;
        return;
    }
    double *Tj = q.T + (int64_t)j * m;
    for (int i = 0; i <= j; ++i) Tj[i] = q.h1[i] + q.h2[i];
    const double hn = sqrt(nn);
    q.beta[j] = hn;
    q.hn[0] = hn;
    if (nn == 0.0) {                                             // gate I
        state[0] = iter;
        state[1] = EIGSH_INVARIANT;
    }
}

// second stage of w.w, one workgroup; runs the small step where no all-reduce follows (gate != 0)
__global__ __launch_bounds__(RT) void eigsh_update_stage2_kernel(const double *__restrict__ partial, int np, EigshSmall q, int j,
                                                                 int m, int64_t iter, int gate, int64_t *__restrict__ state)
{
    if (state[1] != PCG_RUNNING) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) acc = acc + partial[i];
    const double nn = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) {
        q.nn[0] = nn;
        if (gate) eigsh_small_step(q, j, m, nn, iter, state);
    }
}

__global__ void eigsh_small_step_kernel(EigshSmall q, int j, int m, int64_t iter, int64_t *__restrict__ state)
{
    if (threadIdx.x == 0 && state[1] == PCG_RUNNING) eigsh_small_step(q, j, m, q.nn[0], iter, state);
}

// where the small arrays of hp.eigsh live in the solve's one buffer of doubles: which = 0 .. 5 for T, beta, h1, h2, nn, hn;
// which = 6: the buffer's length
HPCLA_API int64_t hpcla_eigsh_small_offset(int ncv, int which)
{
    if (ncv < 1 || ncv > GMRES_MAX_RESTART || which < 0 || which > 6) return -1;
    int64_t off[7];
    eigsh_small_offsets(ncv, off);
    return off[which];
}

// the second pass of column j = ncols - 1: w = w - V h2, nn = w.w (one all-reduce), then the Lanczos small step with gates N, I
HPCLA_API int hpcla_eigsh_update_f64(hpcla_comm_t *comm, const double *V, int64_t ldv, int ncols, const double *h_dev, double *w,
                                     int64_t n, int64_t iter, int ncv, double *small_dev, int64_t *state_dev, void *work,
                                     void *stream)
{
    if (gmres_bad_basis(n, ldv, ncols, ncv) || iter < 1)
        return set_error(HPCLA_ERR_INVALID, "eigsh_update: negative size, odd or short pitch, bad column count or iteration < 1");
    if (!h_dev || !state_dev || !small_dev || !work)
        return set_error(HPCLA_ERR_INVALID, "eigsh_update: null coefficients / state / small arrays / work");
    if (n > 0 && (!V || !w)) return set_error(HPCLA_ERR_INVALID, "eigsh_update: null vector");
    if (misaligned16({V, w})) return set_error(HPCLA_ERR_INVALID, "eigsh_update: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    hipStream_t s = as_stream(stream);
    EigshSmall q;
    eigsh_small_layout(ncv, small_dev, &q);
    gmres_update_kernel<true><<<g, RT, 0, s>>>(V, ldv, ncols, h_dev, w, n, state_dev, partial);
    HPCLA_CHECK_LAUNCH();
    eigsh_update_stage2_kernel<<<1, RT, 0, s>>>(partial, g, q, ncols - 1, ncv, iter, comm ? 0 : 1, state_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, q.nn, 1, 0, stream);
    if (rc) return rc;
    eigsh_small_step_kernel<<<1, 64, 0, s>>>(q, ncols - 1, ncv, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// ---- the Golub-Kahan step of hp.svds (thick-restart bidiagonalisation, full two-sided CGS2; hpcla_svds_steps_*) --------------
// Column j of a cycle of m = ncv columns, iter 1-based over the whole solve, is two halves on two bases: the left half on U
// (j columns: u = A V_j against U_0..U_{j-1}) and the right half on V (j + 1 columns: v = At U_j against V_0..V_j).  Each half
// is gmres_dots, gmres_update (first pass), gmres_dots, then THIS second pass -- gmres_update_kernel<true> as it is (with
// c == 0 columns it is the norm alone) and the small step of that side.  It keeps the projected matrix: B (m x m, column j at
// B + j*m, upper triangle), beta (m):
//   side 0   N   aa != aa  -> status 2 (breakdown), done_iter = iter - 1; nothing of column j is stored
//            B[i, j] = g1[i] + g2[i], i < j;  B[j, j] = dv = sqrt(aa)
//            Z   aa == 0   -> status 4 (invariant), done_iter = iter - 1: j finished triplets, column j of B is stored
//   side 1   N'  bb != bb  -> status 2, done_iter = iter - 1; beta[j] is not stored
//            beta[j] = dv = sqrt(bb)
//            Z'  bb == 0   -> status 4, done_iter = iter: j + 1 finished triplets, beta[j] = 0 is stored
// The host tells Z from Z' by done_iter and beta: with c = p + (done_iter - iterations before the cycle) finished columns the
// gate was Z' when c > p and beta[c - 1] == 0, and Z otherwise (behind Z' at column c - 1 nothing runs, so a Z at column c
// has a beta[c - 1] != 0 of this cycle, and c == p is a cycle whose first left half stopped).
// gmres_next then writes U_j = u / dv or V_{j+1} = v / dv (gated: not behind a stop).
struct SvdsSmall {
    double *B, *beta, *g1, *g2, *h1, *h2, *aa, *bb, *dv;     // B: m x m;  beta, g1, g2, h1, h2: m;  aa, bb, dv: 1
};

static void svds_small_offsets(int m, int64_t off[10])          // off[9]: the buffer's length
{
    const int64_t len[9] = {(int64_t)m * m, m, m, m, m, m, 1, 1, 1};
    off[0] = 0;
    for (int i = 0; i < 9; ++i) off[i + 1] = off[i] + len[i];
}

static void svds_small_layout(int m, double *base, SvdsSmall *q)
{
    int64_t off[10];
    svds_small_offsets(m, off);
    *q = SvdsSmall{base + off[0], base + off[1], base + off[2], base + off[3], base + off[4],
                   base + off[5], base + off[6], base + off[7], base + off[8]};
}

__device__ void svds_small_step(const SvdsSmall &q, int j, int m, int side, double nn, int64_t iter, int64_t *state)
{
    if (nn != nn) {                                              // gates N and N'
        state[0] = iter - 1;
        state[1] = PCG_BREAKDOWN;
        return;
    }
    const double r = sqrt(nn);
    if (side == 0) {
        double *Bj = q.B + (int64_t)j * m;
        for (int i = 0; i < j; ++i) Bj[i] = q.g1[i] + q.g2[i];
        Bj[j] = r;
    } else {
        q.beta[j] = r;
    }
    q.dv[0] = r;
    if (nn == 0.0) {                                             // gates Z and Z'
        state[0] = side == 0 ? iter - 1 : iter;
        state[1] = EIGSH_INVARIANT;
    }
}

// second stage of the norm, one workgroup; runs the small step where no all-reduce follows (gate != 0)
__global__ __launch_bounds__(RT) void svds_update_stage2_kernel(const double *__restrict__ partial, int np, SvdsSmall q, int j,
                                                                int m, int side, int64_t iter, int gate,
                                                                int64_t *__restrict__ state)
{
    if (state[1] != PCG_RUNNING) return;
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += RT) acc = acc + partial[i];
    const double nn = block_reduce<RED_SUM>(acc);
    if (threadIdx.x == 0) {
        (side == 0 ? q.aa : q.bb)[0] = nn;
        if (gate) svds_small_step(q, j, m, side, nn, iter, state);
    }
}

__global__ void svds_small_step_kernel(SvdsSmall q, int j, int m, int side, int64_t iter, int64_t *__restrict__ state)
{
    if (threadIdx.x == 0 && state[1] == PCG_RUNNING) svds_small_step(q, j, m, side, (side == 0 ? q.aa : q.bb)[0], iter, state);
}

// where the small arrays of hp.svds live in the solve's one buffer of doubles: which = 0 .. 8 for B, beta, g1, g2, h1, h2, aa,
// bb, dv; which = 9: the buffer's length
HPCLA_API int64_t hpcla_svds_small_offset(int ncv, int which)
{
    if (ncv < 1 || ncv > GMRES_MAX_RESTART || which < 0 || which > 9) return -1;
    int64_t off[10];
    svds_small_offsets(ncv, off);
    return off[which];
}

// the second pass of one half of column j: w = w - W h, nn = w.w (one all-reduce), then the small step of that side.
// side 0: W = U, ncols = j in 0..ncv-1 (0: the norm and the small step alone);  side 1: W = V, ncols = j + 1 in 1..ncv
HPCLA_API int hpcla_svds_update_f64(hpcla_comm_t *comm, const double *W, int64_t ldw, int ncols, const double *h_dev, double *w,
                                    int64_t n, int64_t iter, int ncv, int side, double *small_dev, int64_t *state_dev,
                                    void *work, void *stream)
{
    if (side != 0 && side != 1) return set_error(HPCLA_ERR_INVALID, "svds_update: side must be 0 (left) or 1 (right)");
    if (n < 0 || ldw < n || (ldw & 1) || ncv < 1 || ncv > GMRES_MAX_RESTART || iter < 1 || ncols < side ||
        ncols > ncv - 1 + side)
        return set_error(HPCLA_ERR_INVALID, "svds_update: negative size, odd or short pitch, bad column count or iteration < 1");
    if (!state_dev || !small_dev || !work || (ncols > 0 && !h_dev))
        return set_error(HPCLA_ERR_INVALID, "svds_update: null coefficients / state / small arrays / work");
    if (n > 0 && (!w || (ncols > 0 && !W))) return set_error(HPCLA_ERR_INVALID, "svds_update: null vector");
    if (misaligned16({W, w})) return set_error(HPCLA_ERR_INVALID, "svds_update: vectors must be 16-byte aligned");
    double *partial = reinterpret_cast<double *>(work);
    const int g = reduce_grid(n);
    const int j = ncols - side;
    hipStream_t s = as_stream(stream);
    SvdsSmall q;
    svds_small_layout(ncv, small_dev, &q);
    gmres_update_kernel<true><<<g, RT, 0, s>>>(W, ldw, ncols, h_dev, w, n, state_dev, partial);
    HPCLA_CHECK_LAUNCH();
    svds_update_stage2_kernel<<<1, RT, 0, s>>>(partial, g, q, j, ncv, side, iter, comm ? 0 : 1, state_dev);
    HPCLA_CHECK_LAUNCH();
    if (!comm) return HPCLA_OK;
    const int rc = allreduce_on(comm, side == 0 ? q.aa : q.bb, 1, 0, stream);
    if (rc) return rc;
    svds_small_step_kernel<<<1, 64, 0, s>>>(q, j, ncv, side, iter, state_dev);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// merge-combine: the five addition kernels of the reference (_copy_a_only_/_copy_b_only_/
// _negate_b_only_/_add_both_/_sub_both_kernel!, src/sparse.jl:1258-1303) as ONE pass over the result:
// entry i of the merged pattern takes a[ia[i]] (ia[i] >= 0) and/or b[ib[i]] (ib[i] >= 0); an entry that
// exists on one side only is COPIED (or negated), never added to zero, exactly like the reference's
// copy kernels (so -0.0 survives).  The result is written contiguously and both source index lists
// are ascending, so all five streams are coalesced; 8 (out) + 2*sizeof(I) (lists) + <= 16 (values)
// bytes per result entry instead of three index-mapped scatter passes.
template <typename I>
__global__ __launch_bounds__(256) void merge_combine_kernel(double *__restrict__ out,
                                                            const double *__restrict__ a,
                                                            const I *__restrict__ ia,
                                                            const double *__restrict__ b,
                                                            const I *__restrict__ ib, int64_t n,
                                                            int subtract)
{
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (; i < n; i += stride) {
        const I ja = ia[i], jb = ib[i];
        double r = 0.0;
        if (ja >= 0 && jb >= 0) {
            const double av = a[ja], bv = b[jb];
            r = subtract ? av - bv : av + bv;
        } else if (ja >= 0) {
            r = a[ja];
        } else if (jb >= 0) {
            const double bv = b[jb];
            r = subtract ? -bv : bv;
        }
        out[i] = r;
    }
}

template <typename I>
static int merge_combine_launch(double *out, const double *a, const I *ia, const double *b, const I *ib,
                                int64_t n, int subtract, void *stream)
{
    if (n < 0 || (subtract != 0 && subtract != 1))
        return set_error(HPCLA_ERR_INVALID, "merge_combine: bad size/mode");
    if (n == 0) return HPCLA_OK;
    if (!out || !a || !b || !ia || !ib) return set_error(HPCLA_ERR_INVALID, "merge_combine: null pointer");
    merge_combine_kernel<I><<<ew_grid(n), 256, 0, as_stream(stream)>>>(out, a, ia, b, ib, n, subtract);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

HPCLA_API int hpcla_merge_combine_f64_i32(double *out, const double *a, const int32_t *ia, const double *b,
                                          const int32_t *ib, int64_t n, int subtract, void *stream)
{
    return merge_combine_launch<int32_t>(out, a, ia, b, ib, n, subtract, stream);
}

HPCLA_API int hpcla_merge_combine_f64_i64(double *out, const double *a, const int64_t *ia, const double *b,
                                          const int64_t *ib, int64_t n, int subtract, void *stream)
{
    return merge_combine_launch<int64_t>(out, a, ia, b, ib, n, subtract, stream);
}

HPCLA_API int hpcla_fill_uniform_f64(double *v, int64_t start, int64_t count, uint64_t seed,
                                     void *stream)
{
    if (count < 0) return set_error(HPCLA_ERR_INVALID, "fill: negative size");
    if (count == 0) return HPCLA_OK;
    if (!v) return set_error(HPCLA_ERR_INVALID, "fill: null pointer");
    fill_uniform_kernel<<<ew_grid(count), 256, 0, as_stream(stream)>>>(v, start, count, seed);
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}
