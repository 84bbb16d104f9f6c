// qr.hip -- communication-avoiding Householder QR (TSQR) of a tall row-major block (hp.qr, hp.lstsq): X = Q R, X n x k, 1 <= k <= 32.
//
// THE TREE IS ONE KERNEL APPLIED TO SHRINKING MATRICES.  A "matrix" is rows of k doubles on a pitch; a "panel" is a run of
// rows_per_panel consecutive rows, owned by one 256-lane workgroup (one lane per row, the row in registers).
//   level 0      the matrix is X, a panel is QR_P = 256 rows.  The panel's Householder reflectors (unit lower trapezoidal: V[r][j]
//                for r > j in panel-local rows) go to the same rows of the caller's Q buffer, which doubles as reflector storage;
//                tau[panel][k] and the panel's k x k triangle (explicit zeros below the diagonal) go to `work`.
//   level l >= 1 the matrix is the level below's triangles, which lie back to back as (nodes * k) rows on pitch k; a panel is
//                F * k rows, F = QR_P / KT triangles (KT = 4, 8, 16 or 32 >= k).  The reflectors overwrite the triangles they
//                were computed from (a panel is loaded whole before anything is stored), tau and the node's triangle are new.
//   until one triangle is left.  A last partial panel, and a panel of fewer than k rows, are zero-padded in registers: a zero
//   row gives sigma contributions of zero, and a column whose sigma is exactly zero gets tau = 0 (the identity).
// Across ranks every rank copies its root triangle into its slot of a zeroed (nranks * k) x k stack and one all-reduce (sum)
// follows: every other rank adds zeros, so each slot arrives bit-exact and the stack is the same on every rank.  Every rank then
// factors the stack with the SAME tree code (level 0 takes any rows, not only triangles), so the root R has the same bits
// everywhere.  D = sign(diag R) (sign(0) = +1), R <- D R.
// Q, top down: the root's k x k "top" is D.  A panel whose top is T forms H_1 .. H_k [T; 0] by applying its reflectors in
// reverse order, in place over the reflectors; the k x k blocks of the result are the tops of its children (upper levels) or
// rows of Q (level 0).  With ranks, block `rank` of the stack's result Q_stack D is the top of the rank's own tree.
//
// PANEL PRIMITIVE (factor), column j = 0 .. k-1, every lane with row r, dlarfg / dlarf:
//   sigma = sum_{r > j} a_rj^2: xor-butterfly inside the wave (every lane ends with the same bits), the four wave partials added
//   in wave order through LDS; a_jj travels in the same LDS exchange (barrier 1).   sigma == 0: tau = 0.  Else
//   alpha = -copysign(sqrt(a_jj^2 + sigma), a_jj);  v_r = a_rj / (a_jj - alpha) (r > j), v_j = 1;  tau = (alpha - a_jj) / alpha.
//   w_c = sum_r v_r a_rc for every c > j: the same butterfly per column, all wave partials written, ONE barrier (barrier 2), each
//   lane adds the four partials per column in wave order;  a_rc = a_rc - v_r * (tau * w_c) for r >= j.
// Products and sums are separately rounded (-ffp-contract=off); every order is fixed by (rows, k), so the same input gives the
// same bits on every call and on every rank.  Form-Q applies H_j the same way to all k columns, one barrier per reflector (the
// wave partials are double-buffered).
// Memory: global <-> registers goes through LDS in two stages of 128 rows with the coalesced (row, column) walk of
// lobpcg_combine, at an odd row stride (a one-lane-one-row global access does not coalesce on a row-major pitch).  LDS per
// workgroup: 128 * (k | 1) * 8 bytes <= 33 KiB, plus 2.1 KiB of partials.  Registers: a row is KT doubles (form-Q: two rows).
// Bytes per row of X: factor 8k read + 8k written (reflectors; nothing written without Q), form-Q 8k read + 8k written.
// In place is safe because a row belongs to one workgroup, which holds its panel in registers before it stores anything.
// No loop in this file waits on memory another workgroup writes: every cross-workgroup dependency is a kernel boundary on the
// caller's stream.  No atomics, no cooperative launch.
#include "common.h"
#include "comm_internal.h"

namespace hpcla {

int allreduce_on(hpcla_comm_t *comm, double *buf, int64_t count, int op, void *stream);  // comm.hip

constexpr int QR_MAX_K = 32;
constexpr int QR_THREADS = 256;
constexpr int QR_P = 256;                      // rows of a level-0 panel: one per lane
constexpr int QR_WAVES = QR_THREADS / 64;
constexpr int QR_STAGE = 128;                  // rows of one LDS staging step
constexpr int QR_MAX_LEVELS = 16;              // 256 * 8^15 rows: more than an int64 pitch can address

static int qr_kt(int k) { return k <= 4 ? 4 : (k <= 8 ? 8 : (k <= 16 ? 16 : 32)); }
static int qr_fan(int k) { return QR_P / qr_kt(k); }

__device__ __forceinline__ double qr_wave_sum(double x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = x + __shfl_xor(x, m, 64);
    return x;
}

// rows [0, nrows) of a panel (global, pitch ld) <-> the lanes' registers a[0 .. k), through LDS in stages of QR_STAGE rows.
// Loading: rows at and past nrows come back as zero.  The caller needs no barrier around either call.
template <int KT>
__device__ __forceinline__ void qr_panel_load(const double *G, int64_t ld, int nrows, int k, double *stage,
                                              double (&a)[KT], int tid)
{
    const int ldl = k | 1;
#pragma unroll
    for (int c = 0; c < KT; ++c) a[c] = 0.0;
    for (int h = 0; h * QR_STAGE < nrows; ++h) {
        const int r0 = h * QR_STAGE, rows = min(QR_STAGE, nrows - r0);
        for (int e = tid; e < rows * k; e += QR_THREADS) {
            const int row = e / k, col = e - row * k;
            stage[row * ldl + col] = G[(int64_t)(r0 + row) * ld + col];
        }
        __syncthreads();
        const int mine = tid - r0;
        if (mine >= 0 && mine < rows) {
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < k) a[c] = stage[mine * ldl + c];
        }
        __syncthreads();
    }
}

template <int KT>
__device__ __forceinline__ void qr_panel_store(double *G, int64_t ld, int nrows, int k, double *stage, const double (&a)[KT], int tid)
{
    const int ldl = k | 1;
    for (int h = 0; h * QR_STAGE < nrows; ++h) {
        const int r0 = h * QR_STAGE, rows = min(QR_STAGE, nrows - r0);
        const int mine = tid - r0;
        if (mine >= 0 && mine < rows) {
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < k) stage[mine * ldl + c] = a[c];
        }
        __syncthreads();
        for (int e = tid; e < rows * k; e += QR_THREADS) {
            const int row = e / k, col = e - row * k;
            G[(int64_t)(r0 + row) * ld + col] = stage[row * ldl + col];
        }
        __syncthreads();
    }
}

// ---- factor: panel p of the matrix `in` (n rows) -> reflectors into V (may be `in` itself, or NULL: R only), tau[p][k], R[p][k][k]
template <int KT>
__global__ __launch_bounds__(QR_THREADS) void qr_factor_kernel(const double *in, int64_t ldin, int64_t n, int rows_per_panel, int k,
                                                               double *V, int64_t ldv, double *__restrict__ tau_out,
                                                               double *__restrict__ R_out)
{
    extern __shared__ __attribute__((aligned(16))) double qr_smem[];
    double *sig = qr_smem;                          // [QR_WAVES] wave partials of sigma, then a_jj
    double *wpart = qr_smem + 8;                    // [QR_WAVES][KT]
    double *stage = wpart + QR_WAVES * KT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t row0 = (int64_t)blockIdx.x * rows_per_panel;
    const int nrows = (int)min((int64_t)rows_per_panel, n - row0);
    double a[KT];
    qr_panel_load<KT>(in + row0 * ldin, ldin, nrows, k, stage, a, tid);

#pragma unroll
    for (int j = 0; j < KT; ++j) {
        if (j < k) {                                 // uniform
            const double below = tid > j ? a[j] : 0.0;
            const double part = qr_wave_sum(below * below);
            if (lane == 0) sig[wave] = part;
            if (tid == j) sig[QR_WAVES] = a[j];
            __syncthreads();
            double sigma = sig[0];
#pragma unroll
            for (int w = 1; w < QR_WAVES; ++w) sigma = sigma + sig[w];
            const double ajj = sig[QR_WAVES];
            double tau = 0.0, alpha = ajj, v = tid == j ? 1.0 : 0.0;
            if (sigma != 0.0) {                      // the exact-zero gate; a NaN sigma takes this branch and propagates
                alpha = -copysign(sqrt(ajj * ajj + sigma), ajj);
                tau = (alpha - ajj) / alpha;
                if (tid > j) v = a[j] / (ajj - alpha);
            }
            if (tid == 0 && tau_out) tau_out[(int64_t)blockIdx.x * k + j] = tau;
            if (tid == j) a[j] = alpha;
            else if (tid > j) a[j] = v;              // the stored reflector (zero where the column was zero)
            if (tau != 0.0) {                        // uniform: every lane holds the same tau
#pragma unroll
                for (int c = j + 1; c < KT; ++c)
                    if (c < k) {
                        const double s = qr_wave_sum(v * a[c]);
                        if (lane == 0) wpart[wave * KT + c] = s;
                    }
            }
            __syncthreads();
            if (tau != 0.0 && tid >= j) {
#pragma unroll
                for (int c = j + 1; c < KT; ++c)
                    if (c < k) {
                        double w = wpart[c];
#pragma unroll
                        for (int q = 1; q < QR_WAVES; ++q) w = w + wpart[q * KT + c];
                        const double t = tau * w;
                        a[c] = a[c] - v * t;
                    }
            }
        }
    }

    if (tid < k) {                                   // the triangle: rows 0 .. k-1 of the panel, zeros below the diagonal
        double *Rp = R_out + (int64_t)blockIdx.x * k * k + tid * k;
#pragma unroll
        for (int c = 0; c < KT; ++c)
            if (c < k) Rp[c] = c >= tid ? a[c] : 0.0;
    }
    if (V) qr_panel_store<KT>(V + row0 * ldv, ldv, nrows, k, stage, a, tid);
}

// reflectors J, J - 1, .. 0 applied to q, J a template argument so that v[J] is a register (a 32-step loop with 32-column bodies
// is past the compiler's full-unroll limit and would index v in scratch memory)
template <int KT, int J>
__device__ __forceinline__ void qr_apply_steps(const double (&v)[KT], double (&q)[KT], int k, const double *__restrict__ tau,
                                               double *wpart, int &buf, int tid, int wave, int lane)
{
    if (J < k) {                                     // uniform
        const double t_j = tau[J];
        if (t_j != 0.0) {                            // uniform
            const double vj = tid > J ? v[J] : (tid == J ? 1.0 : 0.0);
            double *wp = wpart + buf * QR_WAVES * KT;
            buf ^= 1;
#pragma unroll
            for (int c = 0; c < KT; ++c)
                if (c < k) {
                    const double s = qr_wave_sum(vj * q[c]);
                    if (lane == 0) wp[wave * KT + c] = s;
                }
            __syncthreads();
            if (tid >= J) {
#pragma unroll
                for (int c = 0; c < KT; ++c)
                    if (c < k) {
                        double w = wp[c];
#pragma unroll
                        for (int g = 1; g < QR_WAVES; ++g) w = w + wp[g * KT + c];
                        const double t = t_j * w;
                        q[c] = q[c] - vj * t;
                    }
            }
        }
    }
    if constexpr (J > 0) qr_apply_steps<KT, J - 1>(v, q, k, tau, wpart, buf, tid, wave, lane);
}

// ---- form Q: panel p of V (n rows, reflectors as the factor kernel left them) <- H_1 .. H_k [top_p; 0], in place
template <int KT>
__global__ __launch_bounds__(QR_THREADS) void qr_apply_kernel(double *V, int64_t ldv, int64_t n, int rows_per_panel, int k,
                                                              const double *__restrict__ tau_in, const double *__restrict__ tops)
{
    extern __shared__ __attribute__((aligned(16))) double qr_smem[];
    double *wpart = qr_smem;                        // [2][QR_WAVES][KT]
    double *stage = qr_smem + 2 * QR_WAVES * KT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t row0 = (int64_t)blockIdx.x * rows_per_panel;
    const int nrows = (int)min((int64_t)rows_per_panel, n - row0);
    double v[KT], q[KT];
    qr_panel_load<KT>(V + row0 * ldv, ldv, nrows, k, stage, v, tid);
    const double *top = tops + (int64_t)blockIdx.x * k * k;
    const double *tau = tau_in + (int64_t)blockIdx.x * k;
#pragma unroll
    for (int c = 0; c < KT; ++c) q[c] = (c < k && tid < k) ? top[tid * k + c] : 0.0;

    int buf = 0;                                     // the partials alternate between two buffers: one barrier per reflector
    qr_apply_steps<KT, KT - 1>(v, q, k, tau, wpart, buf, tid, wave, lane);
    __syncthreads();                                 // the last partials have been read before the stage is reused
    qr_panel_store<KT>(V + row0 * ldv, ldv, nrows, k, stage, q, tid);
}

// R_dev = D R_root (zeros below the diagonal), top = D, D = sign(diag R_root) with sign(0) = sign(NaN) = +1
__global__ __launch_bounds__(QR_THREADS) void qr_sign_kernel(const double *__restrict__ R_root, int k, double *__restrict__ R_dev,
                                                             double *__restrict__ top)
{
    for (int e = threadIdx.x; e < k * k; e += QR_THREADS) {
        const int r = e / k, c = e - r * k;
        const double d = R_root[r * k + r] < 0.0 ? -1.0 : 1.0;
        R_dev[e] = c >= r ? d * R_root[e] : 0.0;
        top[e] = r == c ? d : 0.0;
    }
}

struct QrLevel {
    double *V;              // the level's matrix: reflectors in place (level 0 of the caller's tree: the Q buffer)
    int64_t ldv, rows;
    int rpp;                // rows per panel
    int64_t panels;
    double *tau, *R;        // [panels][k], [panels][k][k]
};

static size_t qr_lds_bytes(int k, int kt, bool apply)
{
    return ((apply ? 2 * QR_WAVES * kt : 8 + QR_WAVES * kt) + (size_t)QR_STAGE * (size_t)(k | 1)) * sizeof(double);
}

// node counts of the tree over `rows` rows, bottom up; 0 levels for no rows
static int qr_levels(int64_t rows, int k, int64_t *panels)
{
    int L = 0;
    if (rows <= 0) return 0;
    int64_t p = (rows + QR_P - 1) / QR_P;
    panels[L++] = p;
    while (p > 1 && L < QR_MAX_LEVELS) {
        p = (p + qr_fan(k) - 1) / qr_fan(k);
        panels[L++] = p;
    }
    return L;
}

// doubles of tau and triangles of a tree over `rows` rows
static int64_t qr_tree_doubles(int64_t rows, int k)
{
    int64_t panels[QR_MAX_LEVELS], total = 0;
    const int L = qr_levels(rows, k, panels);
    for (int l = 0; l < L; ++l) total += panels[l] * (int64_t)(k + k * k);
    return total;
}

static int qr_launch_factor(const double *in, int64_t ldin, int64_t rows, const QrLevel &lv, bool keep, int k, hipStream_t s)
{
    HPCLA_CHECK_GRID(lv.panels, "qr");
    const int kt = qr_kt(k);
    const size_t lds = qr_lds_bytes(k, kt, false);
    double *V = keep ? lv.V : nullptr;
#define HPCLA_QR_FACTOR(KT) qr_factor_kernel<KT><<<(unsigned)lv.panels, QR_THREADS, lds, s>>>(in, ldin, rows, lv.rpp, k, V, lv.ldv, lv.tau, lv.R)
    if (kt == 4) HPCLA_QR_FACTOR(4);
    else if (kt == 8) HPCLA_QR_FACTOR(8);
    else if (kt == 16) HPCLA_QR_FACTOR(16);
    else HPCLA_QR_FACTOR(32);
#undef HPCLA_QR_FACTOR
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

static int qr_launch_apply(const QrLevel &lv, const double *tops, int k, hipStream_t s)
{
    const int kt = qr_kt(k);
    const size_t lds = qr_lds_bytes(k, kt, true);
#define HPCLA_QR_APPLY(KT) qr_apply_kernel<KT><<<(unsigned)lv.panels, QR_THREADS, lds, s>>>(lv.V, lv.ldv, lv.rows, lv.rpp, k, lv.tau, tops)
    if (kt == 4) HPCLA_QR_APPLY(4);
    else if (kt == 8) HPCLA_QR_APPLY(8);
    else if (kt == 16) HPCLA_QR_APPLY(16);
    else HPCLA_QR_APPLY(32);
#undef HPCLA_QR_APPLY
    HPCLA_CHECK_LAUNCH();
    return HPCLA_OK;
}

// Lays the tree over (X, rows) out in `work` (advancing it) and factors it bottom up.  V0 / ldv0: where level 0 keeps its
// reflectors (ignored without keep).  Returns the level count in *L_out; the root triangle is lv[L - 1].R.
static int qr_factor_tree(const double *X, int64_t ldx, int64_t rows, int k, double *V0, int64_t ldv0, bool keep, double **work,
                          QrLevel *lv, int *L_out, hipStream_t s)
{
    int64_t panels[QR_MAX_LEVELS];
    const int L = qr_levels(rows, k, panels);
    for (int l = 0; l < L; ++l) {
        lv[l].panels = panels[l];
        lv[l].tau = *work;
        lv[l].R = *work + panels[l] * k;
        *work += panels[l] * (int64_t)(k + k * k);
        if (l == 0) {
            lv[l].V = V0, lv[l].ldv = ldv0, lv[l].rows = rows, lv[l].rpp = QR_P;
        } else {
            lv[l].V = lv[l - 1].R, lv[l].ldv = k, lv[l].rows = panels[l - 1] * k, lv[l].rpp = qr_fan(k) * k;
        }
        const int rc = qr_launch_factor(l == 0 ? X : lv[l].V, l == 0 ? ldx : (int64_t)k, lv[l].rows, lv[l], keep, k, s);
        if (rc != HPCLA_OK) return rc;
    }
    *L_out = L;
    return HPCLA_OK;
}

// top down: the root's top is `top`; level l's tops are level l + 1's result blocks
static int qr_apply_tree(const QrLevel *lv, int L, const double *top, int k, hipStream_t s)
{
    for (int l = L - 1; l >= 0; --l) {
        const int rc = qr_launch_apply(lv[l], l == L - 1 ? top : lv[l + 1].V, k, s);
        if (rc != HPCLA_OK) return rc;
    }
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int hpcla_qr_panel_rows(void) { return QR_P; }

HPCLA_API int hpcla_qr_fan(int k) { return k >= 1 && k <= QR_MAX_K ? qr_fan(k) : 0; }

HPCLA_API int64_t hpcla_qr_work_bytes(int64_t nloc, int k, int nranks, int want_q)
{
    if (k < 1 || k > QR_MAX_K || nloc < 0 || nranks < 1) return 8;
    // the rank's tree, a zero triangle for a rank without rows, the sign matrix, the stack and its tree
    int64_t d = qr_tree_doubles(nloc, k) + 2 * (int64_t)k * k;
    if (nranks > 1) d += (int64_t)nranks * k * k + qr_tree_doubles((int64_t)nranks * k, k);
    return d * (int64_t)sizeof(double);
}

HPCLA_API int hpcla_qr_f64(hpcla_comm_t *comm, const double *X, int64_t ldx, int64_t nloc, int k, double *Q, int64_t ldq,
                           double *R_dev, double *work, void *stream)
{
    if (k < 1 || k > QR_MAX_K) return set_error(HPCLA_ERR_INVALID, "qr: needs 1 <= k <= 32");
    if (nloc < 0 || ldx < k || (Q && ldq < k)) return set_error(HPCLA_ERR_INVALID, "qr: negative size, or a pitch shorter than k");
    if (!R_dev || !work) return set_error(HPCLA_ERR_INVALID, "qr: null R or work");
    if (nloc > 0 && !X) return set_error(HPCLA_ERR_INVALID, "qr: null X");
    if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(R_dev) |
         reinterpret_cast<uintptr_t>(work)) & 7)
        return set_error(HPCLA_ERR_INVALID, "qr: every array must be 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const int nranks = comm ? comm->nranks : 1, rank = comm ? comm->rank : 0;
    const bool keep = Q != nullptr;
    const int64_t kk = (int64_t)k * k;
    double *w = work;
    double *zero_tri = w, *top = w + kk;
    w += 2 * kk;

    QrLevel mine[QR_MAX_LEVELS], stack[QR_MAX_LEVELS];
    int L = 0, Ls = 0;
    int rc = qr_factor_tree(X, ldx, nloc, k, Q, ldq, keep, &w, mine, &L, s);
    if (rc != HPCLA_OK) return rc;
    const double *root = L ? mine[L - 1].R : zero_tri;
    if (!L) HPCLA_CHECK_HIP(hipMemsetAsync(zero_tri, 0, (size_t)kk * sizeof(double), s));

    double *S = nullptr;
    if (nranks > 1) {
        S = w;
        w += nranks * kk;
        HPCLA_CHECK_HIP(hipMemsetAsync(S, 0, (size_t)(nranks * kk) * sizeof(double), s));
        HPCLA_CHECK_HIP(hipMemcpyAsync(S + rank * kk, root, (size_t)kk * sizeof(double), hipMemcpyDeviceToDevice, s));
        rc = allreduce_on(comm, S, nranks * kk, 0, stream);
        if (rc != HPCLA_OK) return rc;
        rc = qr_factor_tree(S, k, (int64_t)nranks * k, k, S, k, keep, &w, stack, &Ls, s);
        if (rc != HPCLA_OK) return rc;
        root = stack[Ls - 1].R;
    }
    qr_sign_kernel<<<1, QR_THREADS, 0, s>>>(root, k, R_dev, top);
    HPCLA_CHECK_LAUNCH();
    if (!keep) return HPCLA_OK;
    const double *my_top = top;
    if (nranks > 1) {
        rc = qr_apply_tree(stack, Ls, top, k, s);
        if (rc != HPCLA_OK) return rc;
        my_top = S + rank * kk;                      // this rank's block of Q_stack D
    }
    return qr_apply_tree(mine, L, my_top, k, s);
}
