// solvers.hip -- the host-side iteration loops of the Krylov solvers and eigensolvers: hp.cg (plain, Jacobi, FSAI),
// hp.bicgstab, hp.lsqr, hp.minres, hp.gmres, hp.eigsh, hp.svds.
//
// Host code only, no kernel.  Each loop is a chain of the library's own exported step entries (vecops.hip, eigsh.hip)
// with a distributed product between them (spmv_dist / spmv_dist_dot: spmv_dist.h, defined in comm.hip), enqueued on the
// caller's stream without returning to the host language in between.  Each section's comment states the order of its
// launches and gates; the tests restate the loops in Python and compare bit for bit.
#include "solver_slots.h"
#include "spmv_dist.h"

using namespace hpcla;

// ---- k fused CG iterations in ONE host call ----------------------------------------------------------
// The iteration a caller composes from A*p, dot, the broadcasts and norm (the reference has no Krylov
// solver: src/sparse.jl:2096-2128, src/vectors.jl:798-812, 1203-1226, 758-765), enqueued `iters` times on
// `stream` without returning to the host language in between: per iteration the launches of
// hpcla_spmv_dist_dot_* (Ap = A p, pAp), hpcla_cg_residual_f64 (r -= a Ap, rr') and hpcla_cg_direction_f64
// (x += a p, p = r + (rr'/rr) p) -- the same kernels with the same arguments as the three separate calls,
// hence the same bits.  rr_hist_dev[j] holds sum r_j^2: [0] on entry, [1..iters] written here.
template <typename I>
static int cg_iterations_impl(const SpmvBlock<I> &a, hpcla_comm_t *comm, double *x, double *r, double *p, double *Ap,
                              double *rr_hist_dev, double *pAp_dev, void *dot_work, void *reduce_work, int iters, void *stream)
{
    const int64_t nrows = a.nrows;
    if (iters < 0) return set_error(HPCLA_ERR_INVALID, "cg_iterations: negative iteration count");
    if (!rr_hist_dev || !pAp_dev || !dot_work || !reduce_work)
        return set_error(HPCLA_ERR_INVALID, "cg_iterations: null scalar / work buffer");
    if (nrows > 0 && (!x || !r || !p || !Ap)) return set_error(HPCLA_ERR_INVALID, "cg_iterations: null vector");
    for (int j = 0; j < iters; ++j) {
        double *rr = rr_hist_dev + j;
        int rc = spmv_dist_dot(a, comm, p, nrows, Ap, pAp_dev, dot_work, stream);
        if (rc) return rc;
        rc = hpcla_cg_residual_f64(comm, 1.0, rr, pAp_dev, Ap, r, nrows, rr + 1, reduce_work, stream);
        if (rc) return rc;
        rc = hpcla_cg_direction_f64(1.0, rr, pAp_dev, 1.0, rr + 1, rr, r, x, p, nrows, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

HPCLA_API int hpcla_cg_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                          const int32_t *colval_split, const double *nzval, int64_t nrows,
                                          int64_t nnz, int index_base, const int32_t *interior_blocks,
                                          int64_t n_interior, const int32_t *boundary_blocks, int64_t n_boundary,
                                          double *x, double *r, double *p, double *Ap, double *rr_hist_dev,
                                          double *pAp_dev, void *dot_work, void *reduce_work, int iters,
                                          void *stream)
{
    return cg_iterations_impl<int32_t>({plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base, interior_blocks,
                                        n_interior, boundary_blocks, n_boundary},
                                       comm, x, r, p, Ap, rr_hist_dev, pAp_dev, dot_work, reduce_work, iters, stream);
}

HPCLA_API int hpcla_cg_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                          const int64_t *colval_split, const double *nzval, int64_t nrows,
                                          int64_t nnz, int index_base, const int32_t *interior_blocks,
                                          int64_t n_interior, const int32_t *boundary_blocks, int64_t n_boundary,
                                          double *x, double *r, double *p, double *Ap, double *rr_hist_dev,
                                          double *pAp_dev, void *dot_work, void *reduce_work, int iters,
                                          void *stream)
{
    return cg_iterations_impl<int64_t>({plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base, interior_blocks,
                                        n_interior, boundary_blocks, n_boundary},
                                       comm, x, r, p, Ap, rr_hist_dev, pAp_dev, dot_work, reduce_work, iters, stream);
}

// ---- a chunk of gated, diagonally preconditioned CG iterations in ONE host call (the solver, hp.cg) -------------
// Iteration j = first_iter .. first_iter + iters - 1 (1-based over the whole solve), in this order:
//   1. Ap = A p, pAp      hpcla_spmv_dist_dot_* -- always executed, not gated (the SpMV kernels know nothing of the solve)
//   2. gate A             running and !(pAp > 0): status = breakdown, done_iter = j - 1
//   3. r -= a Ap          gated; partials of sum r^2 and sum r (dinv r), their second stage, ONE all-reduce of the pair
//   4. gate B             running and sum r_j^2 <= thr: status = converged, done_iter = j
//   5. x += a p, p = dinv r + b p    gated, still runs for done_iter == j (the deferred x update)
// Gate A is the residual kernel's own predicate and is recorded by the single-workgroup second stage; gate B is folded
// into that second stage where no all-reduce follows it (comm == NULL), else it is one 64-lane launch behind the
// all-reduce.  hist_dev[2 j], hist_dev[2 j + 1] = sum r_j^2, sum r_j (dinv r_j): the pair is all-reduced in place.
template <typename I>
static int pcg_iterations_impl(const SpmvBlock<I> &a, hpcla_comm_t *comm, const double *dinv, double *x, double *r, double *p,
                               double *Ap, double *hist_dev, double *pAp_dev, void *dot_work, void *pcg_work,
                               int64_t first_iter, int iters, void *stream)
{
    const int64_t nrows = a.nrows;
    if (iters < 0 || first_iter < 1) return set_error(HPCLA_ERR_INVALID, "pcg_iterations: negative count or first_iter < 1");
    if (!hist_dev || !pAp_dev || !dot_work || !pcg_work)
        return set_error(HPCLA_ERR_INVALID, "pcg_iterations: null scalar / work buffer");
    if (nrows > 0 && (!x || !r || !p || !Ap)) return set_error(HPCLA_ERR_INVALID, "pcg_iterations: null vector");
    int64_t *state = solver_state(pcg_work, hpcla_pcg_work_bytes());
    for (int64_t j = first_iter; j < first_iter + iters; ++j) {
        double *prev = hist_dev + 2 * (j - 1), *cur = hist_dev + 2 * j;
        int rc = spmv_dist_dot(a, comm, p, nrows, Ap, pAp_dev, dot_work, stream);
        if (rc) return rc;
        rc = hpcla_pcg_residual_f64(comm, prev + 1, pAp_dev, Ap, dinv, r, nrows, j, state, cur, pcg_work, stream);
        if (rc) return rc;
        rc = hpcla_pcg_direction_f64(prev + 1, pAp_dev, cur + 1, prev + 1, r, dinv, x, p, nrows, j, state, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

HPCLA_API int hpcla_pcg_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                           const int32_t *colval_split, const int16_t *cols16,
                                           const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows,
                                           int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                           const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, double *x,
                                           double *r, double *p, double *Ap, double *hist_dev, double *pAp_dev,
                                           void *dot_work, void *pcg_work, int64_t first_iter, int iters, void *stream)
{
    return pcg_iterations_impl<int32_t>({plan, rowptr, colval_split, cols16, patterns, nzval, nrows, nnz, index_base, interior_blocks,
                                         n_interior, boundary_blocks, n_boundary},
                                        comm, dinv, x, r, p, Ap, hist_dev, pAp_dev, dot_work, pcg_work, first_iter, iters, stream);
}

HPCLA_API int hpcla_pcg_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                           const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                           int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                           const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, double *x,
                                           double *r, double *p, double *Ap, double *hist_dev, double *pAp_dev,
                                           void *dot_work, void *pcg_work, int64_t first_iter, int iters, void *stream)
{
    return pcg_iterations_impl<int64_t>({plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base, interior_blocks,
                                         n_interior, boundary_blocks, n_boundary},
                                        comm, dinv, x, r, p, Ap, hist_dev, pAp_dev, dot_work, pcg_work, first_iter, iters, stream);
}

// ---- the same chunk with M = Gt G, a factorised sparse approximate inverse (hp.cg with M = hp.fsai(A)) -----------------
// G and Gt are matrices with plans of their own.  Iteration j, in this order:
//   1. Ap = A p, pAp      as above
//   2. gate A, r -= a Ap, sum r^2, gate B     hpcla_pcg_residual_f64 with dinv == NULL (the pair's second slot is rewritten by 5)
//   3. u = G r            hpcla_spmv_dist_* on G's plan  -- always executed, not gated
//   4. z = Gt u           the same on Gt's plan          -- always executed
//   5. rz = sum u^2       hpcla_nrm2sq_f64 into hist_dev[2 j + 1], one all-reduce: r.M r, never negative -- always executed
//   6. x += a p, p = z + b p    hpcla_pcg_direction_f64 with z in place of r and dinv == NULL, gated
// Behind the deciding iteration r is frozen, so 3-5 recompute what they computed and write pairs nobody reads.
template <typename I>
static int pcg_fsai_iterations_impl(hpcla_comm_t *comm, const SpmvBlock<I> &a, const SpmvBlock<I> &g,
                                    const SpmvBlock<I> &gt, double *x, double *r, double *p, double *Ap, double *u, double *z,
                                    double *hist_dev, double *pAp_dev, void *dot_work, void *pcg_work, int64_t first_iter,
                                    int iters, void *stream)
{
    if (iters < 0 || first_iter < 1)
        return set_error(HPCLA_ERR_INVALID, "pcg_fsai_iterations: negative count or first_iter < 1");
    if (!hist_dev || !pAp_dev || !dot_work || !pcg_work)
        return set_error(HPCLA_ERR_INVALID, "pcg_fsai_iterations: null scalar / work buffer");
    const int64_t n = a.nrows;
    if (g.nrows != n || gt.nrows != n) return set_error(HPCLA_ERR_INVALID, "pcg_fsai_iterations: G and Gt must have A's rows");
    if (n > 0 && (!x || !r || !p || !Ap || !u || !z)) return set_error(HPCLA_ERR_INVALID, "pcg_fsai_iterations: null vector");
    int64_t *state = solver_state(pcg_work, hpcla_pcg_work_bytes());
    for (int64_t j = first_iter; j < first_iter + iters; ++j) {
        double *prev = hist_dev + 2 * (j - 1), *cur = hist_dev + 2 * j;
        int rc = spmv_dist_dot(a, comm, p, n, Ap, pAp_dev, dot_work, stream);
        if (rc) return rc;
        rc = hpcla_pcg_residual_f64(comm, prev + 1, pAp_dev, Ap, nullptr, r, n, j, state, cur, pcg_work, stream);
        if (rc) return rc;
        rc = spmv_dist(g, r, n, u, stream);
        if (rc) return rc;
        rc = spmv_dist(gt, u, n, z, stream);
        if (rc) return rc;
        rc = hpcla_nrm2sq_f64(comm, u, n, cur + 1, pcg_work, stream);
        if (rc) return rc;
        rc = hpcla_pcg_direction_f64(prev + 1, pAp_dev, cur + 1, prev + 1, z, nullptr, x, p, n, j, state, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

HPCLA_API int hpcla_pcg_fsai_iterations_f64_i32(
    hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int32_t *rowptr, const int32_t *colval_split, const int16_t *cols16,
    const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows, int64_t nnz, int index_base,
    const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks, int64_t n_boundary,
    hpcla_halo_plan_t *plan_g, const int32_t *rowptr_g, const int32_t *colval_split_g, const int16_t *cols16_g,
    const hpcla_block_patterns_t *patterns_g, const double *nzval_g, int64_t nrows_g, int64_t nnz_g, int index_base_g,
    const int32_t *interior_blocks_g, int64_t n_interior_g, const int32_t *boundary_blocks_g, int64_t n_boundary_g,
    hpcla_halo_plan_t *plan_t, const int32_t *rowptr_t, const int32_t *colval_split_t, const int16_t *cols16_t,
    const hpcla_block_patterns_t *patterns_t, const double *nzval_t, int64_t nrows_t, int64_t nnz_t, int index_base_t,
    const int32_t *interior_blocks_t, int64_t n_interior_t, const int32_t *boundary_blocks_t, int64_t n_boundary_t, double *x,
    double *r, double *p, double *Ap, double *u, double *z, double *hist_dev, double *pAp_dev, void *dot_work, void *pcg_work,
    int64_t first_iter, int iters, void *stream)
{
    const SpmvBlock<int32_t> a{plan, rowptr, colval_split, cols16, patterns, nzval, nrows, nnz, index_base, interior_blocks,
                               n_interior, boundary_blocks, n_boundary};
    const SpmvBlock<int32_t> g{plan_g, rowptr_g, colval_split_g, cols16_g, patterns_g, nzval_g, nrows_g, nnz_g, index_base_g,
                               interior_blocks_g, n_interior_g, boundary_blocks_g, n_boundary_g};
    const SpmvBlock<int32_t> gt{plan_t, rowptr_t, colval_split_t, cols16_t, patterns_t, nzval_t, nrows_t, nnz_t, index_base_t,
                                interior_blocks_t, n_interior_t, boundary_blocks_t, n_boundary_t};
    return pcg_fsai_iterations_impl<int32_t>(comm, a, g, gt, x, r, p, Ap, u, z, hist_dev, pAp_dev, dot_work, pcg_work, first_iter,
                                             iters, stream);
}

HPCLA_API int hpcla_pcg_fsai_iterations_f64_i64(
    hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int64_t *rowptr, const int64_t *colval_split, const double *nzval,
    int64_t nrows, int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
    const int32_t *boundary_blocks, int64_t n_boundary, hpcla_halo_plan_t *plan_g, const int64_t *rowptr_g,
    const int64_t *colval_split_g, const double *nzval_g, int64_t nrows_g, int64_t nnz_g, int index_base_g,
    const int32_t *interior_blocks_g, int64_t n_interior_g, const int32_t *boundary_blocks_g, int64_t n_boundary_g,
    hpcla_halo_plan_t *plan_t, const int64_t *rowptr_t, const int64_t *colval_split_t, const double *nzval_t, int64_t nrows_t,
    int64_t nnz_t, int index_base_t, const int32_t *interior_blocks_t, int64_t n_interior_t, const int32_t *boundary_blocks_t,
    int64_t n_boundary_t, double *x, double *r, double *p, double *Ap, double *u, double *z, double *hist_dev, double *pAp_dev,
    void *dot_work, void *pcg_work, int64_t first_iter, int iters, void *stream)
{
    const SpmvBlock<int64_t> a{plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base, interior_blocks,
                               n_interior, boundary_blocks, n_boundary};
    const SpmvBlock<int64_t> g{plan_g, rowptr_g, colval_split_g, nullptr, nullptr, nzval_g, nrows_g, nnz_g, index_base_g,
                               interior_blocks_g, n_interior_g, boundary_blocks_g, n_boundary_g};
    const SpmvBlock<int64_t> gt{plan_t, rowptr_t, colval_split_t, nullptr, nullptr, nzval_t, nrows_t, nnz_t, index_base_t,
                                interior_blocks_t, n_interior_t, boundary_blocks_t, n_boundary_t};
    return pcg_fsai_iterations_impl<int64_t>(comm, a, g, gt, x, r, p, Ap, u, z, hist_dev, pAp_dev, dot_work, pcg_work, first_iter,
                                             iters, stream);
}

// ---- a chunk of gated BiCGStab iterations in ONE host call (the solver, hp.bicgstab) ------------------------------
// Right-preconditioned BiCGStab, K = identity (dinv == NULL: ph is p, sh is s) or dinv .*.  Iteration j = first_iter ..
// first_iter + iters - 1 (1-based over the whole solve), in this order (the gates and the bytes: csrc/vecops.hip):
//   1. v = A ph                     hpcla_spmv_dist_* -- always executed, not gated, no dot partials
//   2. rv = rhat.v, gate A          hpcla_bicg_dot_f64: one all-reduce [rv]
//   3. s = r - a v  [sh = dinv s]   hpcla_bicg_s_f64
//   4. t = A sh                     the SpMV again
//   5. ts, tt, ss, gates S and T    hpcla_bicg_tts_f64: one all-reduce of the triple
//   6. x, r, rr, rho', gates B, O   hpcla_bicg_xr_f64: one all-reduce of the pair (the half-step form behind gate S; its gate,
//                                   behind the all-reduce, then stores ss as the pair's first entry)
//   7. p = r + b (p - w v)  [ph]    hpcla_bicg_p_f64
// One rank: 2 SpMV + 8 launches (every gate is folded into a second stage).  N ranks: + 3 window all-reduces and 3 64-lane
// gate launches.  hist_dev[2 j], hist_dev[2 j + 1] = sum r_j^2 (sum s_j^2 for a half-step stop), rhat.r_j: the pair is
// all-reduced in place and its second entry is the rho of iteration j + 1.  scal_dev: rv, ts, tt, ss.
template <typename I>
static int bicgstab_iterations_impl(const SpmvBlock<I> &a, hpcla_comm_t *comm, const double *dinv, double *x, double *r,
                                    const double *rhat, double *p, double *ph, double *v, double *s, double *sh, double *t,
                                    double *hist_dev, double *scal_dev, void *work, int64_t first_iter, int iters, void *stream)
{
    const int64_t nrows = a.nrows;
    if (iters < 0 || first_iter < 1)
        return set_error(HPCLA_ERR_INVALID, "bicgstab_iterations: negative count or first_iter < 1");
    if (nrows < 0 || a.nnz < 0) return set_error(HPCLA_ERR_INVALID, "bicgstab_iterations: negative size");
    if (!hist_dev || !scal_dev || !work) return set_error(HPCLA_ERR_INVALID, "bicgstab_iterations: null scalar / work buffer");
    if (nrows > 0 && (!x || !r || !rhat || !p || !v || !s || !t || (dinv && (!ph || !sh))))
        return set_error(HPCLA_ERR_INVALID, "bicgstab_iterations: null vector");
    if (misaligned16({x, r, rhat, p, v, s, t, dinv, dinv ? ph : nullptr, dinv ? sh : nullptr}))
        return set_error(HPCLA_ERR_INVALID, "bicgstab_iterations: vectors must be 16-byte aligned");
    int64_t *state = solver_state(work, hpcla_bicgstab_work_bytes());
    double *in1 = dinv ? ph : p, *in2 = dinv ? sh : s;
    double *rv = scal_dev, *triple = scal_dev + 1;
    for (int64_t j = first_iter; j < first_iter + iters; ++j) {
        double *prev = hist_dev + 2 * (j - 1), *cur = hist_dev + 2 * j;
        int rc = spmv_dist(a, in1, nrows, v, stream);
        if (rc) return rc;
        rc = hpcla_bicg_dot_f64(comm, rhat, v, nrows, j, prev + 1, state, rv, work, stream);
        if (rc) return rc;
        rc = hpcla_bicg_s_f64(prev + 1, rv, r, v, dinv, s, dinv ? sh : nullptr, nrows, j, state, stream);
        if (rc) return rc;
        rc = spmv_dist(a, in2, nrows, t, stream);
        if (rc) return rc;
        rc = hpcla_bicg_tts_f64(comm, t, s, nrows, j, state, triple, work, stream);
        if (rc) return rc;
        rc = hpcla_bicg_xr_f64(comm, prev + 1, rv, triple, in1, dinv ? sh : nullptr, s, t, rhat, x, r, nrows, j, state, cur,
                               work, stream);
        if (rc) return rc;
        rc = hpcla_bicg_p_f64(cur + 1, prev + 1, rv, triple, r, v, dinv, p, dinv ? ph : nullptr, nrows, j, state, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

HPCLA_API int hpcla_bicgstab_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                                const int32_t *colval_split, const int16_t *cols16,
                                                const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows,
                                                int64_t nnz, int index_base, const int32_t *interior_blocks,
                                                int64_t n_interior, const int32_t *boundary_blocks, int64_t n_boundary,
                                                const double *dinv, double *x, double *r, const double *rhat, double *p,
                                                double *ph, double *v, double *s, double *sh, double *t, double *hist_dev,
                                                double *scal_dev, void *work, int64_t first_iter, int iters, void *stream)
{
    return bicgstab_iterations_impl<int32_t>({plan, rowptr, colval_split, cols16, patterns, nzval, nrows, nnz, index_base,
                                              interior_blocks, n_interior, boundary_blocks, n_boundary},
                                             comm, dinv, x, r, rhat, p, ph, v, s, sh, t, hist_dev, scal_dev, work, first_iter, iters,
                                             stream);
}

HPCLA_API int hpcla_bicgstab_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                                const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                                int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                                const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv,
                                                double *x, double *r, const double *rhat, double *p, double *ph, double *v,
                                                double *s, double *sh, double *t, double *hist_dev, double *scal_dev,
                                                void *work, int64_t first_iter, int iters, void *stream)
{
    return bicgstab_iterations_impl<int64_t>({plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base,
                                              interior_blocks, n_interior, boundary_blocks, n_boundary},
                                             comm, dinv, x, r, rhat, p, ph, v, s, sh, t, hist_dev, scal_dev, work, first_iter, iters,
                                             stream);
}

// ---- a chunk of gated LSQR iterations in ONE host call (the solver, hp.lsqr) ---------------------------------------
// min |A x - b|^2 + damp^2 |x|^2 for A of any shape m x n, At its materialised transpose (a matrix and a plan of its own).
// Iteration j = first_iter .. first_iter + iters - 1 (1-based over the whole solve), in this order (the scalars, the gates and
// the bytes: csrc/vecops.hip):
//   1. tu = A vh                    hpcla_spmv_dist_* on A's plan -- always executed, not gated
//   2. uh, uu                       hpcla_lsqr_u_f64: one all-reduce [uu]
//   3. tv = At uh                   the SpMV on At's plan -- always executed
//   4. vh, vv, the step, the gates  hpcla_lsqr_v_f64: gate U, one all-reduce [vv], then the one-thread step
//   5. x += t1 w, w                 hpcla_lsqr_xw_f64 (x only in the iteration that stopped)
// One rank: 2 SpMV + 5 launches (the step is folded into vv's second stage).  N ranks: + 2 window all-reduces and one 64-lane
// step launch.  hist_dev[2 j], hist_dev[2 j + 1] = |rbar_j|^2, |Abar' rbar_j|^2 of the recurrences: formed from global
// scalars on every rank, never all-reduced.
template <typename I>
static int lsqr_iterations_impl(hpcla_comm_t *comm, const SpmvBlock<I> &a, const SpmvBlock<I> &at, double *x, double *uh,
                                double *vh, double *w, double *tu, double *tv, double *hist_dev, double *scal_dev, void *work,
                                int64_t first_iter, int iters, void *stream)
{
    const int64_t nrows = a.nrows, nrows_t = at.nrows;
    if (iters < 0 || first_iter < 1) return set_error(HPCLA_ERR_INVALID, "lsqr_iterations: negative count or first_iter < 1");
    if (nrows < 0 || a.nnz < 0 || nrows_t < 0 || at.nnz < 0) return set_error(HPCLA_ERR_INVALID, "lsqr_iterations: negative size");
    if (!hist_dev || !scal_dev || !work) return set_error(HPCLA_ERR_INVALID, "lsqr_iterations: null scalar / work buffer");
    if ((nrows > 0 && (!uh || !tu)) || (nrows_t > 0 && (!x || !vh || !w || !tv)))
        return set_error(HPCLA_ERR_INVALID, "lsqr_iterations: null vector");
    if (misaligned16({x, uh, vh, w, tu, tv})) return set_error(HPCLA_ERR_INVALID, "lsqr_iterations: vectors must be 16-byte aligned");
    int64_t *state = solver_state(work, hpcla_lsqr_work_bytes());
    for (int64_t j = first_iter; j < first_iter + iters; ++j) {
        int rc = spmv_dist(a, vh, nrows_t, tu, stream);
        if (rc) return rc;
        rc = hpcla_lsqr_u_f64(comm, scal_dev, tu, uh, nrows, j, state, work, stream);
        if (rc) return rc;
        rc = spmv_dist(at, uh, nrows, tv, stream);
        if (rc) return rc;
        rc = hpcla_lsqr_v_f64(comm, scal_dev, tv, vh, nrows_t, j, state, hist_dev + 2 * j, work, stream);
        if (rc) return rc;
        rc = hpcla_lsqr_xw_f64(scal_dev, vh, x, w, nrows_t, j, state, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

HPCLA_API int hpcla_lsqr_iterations_f64_i32(hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int32_t *rowptr,
                                            const int32_t *colval_split, const int16_t *cols16,
                                            const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows,
                                            int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                            const int32_t *boundary_blocks, int64_t n_boundary, hpcla_halo_plan_t *plan_t,
                                            const int32_t *rowptr_t, const int32_t *colval_split_t, const int16_t *cols16_t,
                                            const hpcla_block_patterns_t *patterns_t, const double *nzval_t, int64_t nrows_t,
                                            int64_t nnz_t, int index_base_t, const int32_t *interior_blocks_t,
                                            int64_t n_interior_t, const int32_t *boundary_blocks_t, int64_t n_boundary_t,
                                            double *x, double *uh, double *vh, double *w, double *tu, double *tv,
                                            double *hist_dev, double *scal_dev, void *work, int64_t first_iter, int iters,
                                            void *stream)
{
    return lsqr_iterations_impl<int32_t>(comm,
                                         {plan, rowptr, colval_split, cols16, patterns, nzval, nrows, nnz, index_base,
                                          interior_blocks, n_interior, boundary_blocks, n_boundary},
                                         {plan_t, rowptr_t, colval_split_t, cols16_t, patterns_t, nzval_t, nrows_t, nnz_t,
                                          index_base_t, interior_blocks_t, n_interior_t, boundary_blocks_t, n_boundary_t},
                                         x, uh, vh, w, tu, tv, hist_dev, scal_dev, work, first_iter, iters, stream);
}

HPCLA_API int hpcla_lsqr_iterations_f64_i64(hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int64_t *rowptr,
                                            const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                            int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                            const int32_t *boundary_blocks, int64_t n_boundary, hpcla_halo_plan_t *plan_t,
                                            const int64_t *rowptr_t, const int64_t *colval_split_t, const double *nzval_t,
                                            int64_t nrows_t, int64_t nnz_t, int index_base_t,
                                            const int32_t *interior_blocks_t, int64_t n_interior_t,
                                            const int32_t *boundary_blocks_t, int64_t n_boundary_t, double *x, double *uh,
                                            double *vh, double *w, double *tu, double *tv, double *hist_dev, double *scal_dev,
                                            void *work, int64_t first_iter, int iters, void *stream)
{
    return lsqr_iterations_impl<int64_t>(comm,
                                         {plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base,
                                          interior_blocks, n_interior, boundary_blocks, n_boundary},
                                         {plan_t, rowptr_t, colval_split_t, nullptr, nullptr, nzval_t, nrows_t, nnz_t,
                                          index_base_t, interior_blocks_t, n_interior_t, boundary_blocks_t, n_boundary_t},
                                         x, uh, vh, w, tu, tv, hist_dev, scal_dev, work, first_iter, iters, stream);
}

// ---- a chunk of gated MINRES iterations in ONE host call (the solver, hp.minres) ------------------------------------
// A x = b for a symmetric, possibly indefinite A, M = identity (dinv == NULL: y is r) or dinv .*.  Iteration j = first_iter ..
// first_iter + iters - 1 (1-based over the whole solve), in this order (the scalars, the gates and the bytes: csrc/vecops.hip):
//   1. t = A y, yt = y.t            hpcla_spmv_dist_dot_* -- always executed, not gated; one all-reduce [yt]
//   2. rn, [yn,] bb, the step       hpcla_minres_r_f64: one all-reduce [bb], then the one-thread step with gates N, G, C
//   3. w, x += phi w                hpcla_minres_xw_f64 (still runs in the iteration that converged)
// The buffers rotate by the parity of j, so a chunk may start at any iteration: the operand y and r2 are buffer (j - 1) & 1,
// rn and yn overwrite buffer j & 1 (r1 and the y before); w2 is buffer (j - 1) & 1 and the new w overwrites w1, buffer j & 1.
// One rank: SpMV + dot stage + 3 launches (the step is folded into bb's second stage).  N ranks: + 2 window all-reduces and
// one 64-lane step launch.  hist_dev[2 j], hist_dev[2 j + 1] = phibar_j^2, beta_{j+1}^2: formed from global scalars on every
// rank, never all-reduced.
template <typename I>
static int minres_iterations_impl(const SpmvBlock<I> &a, hpcla_comm_t *comm, const double *dinv, double *x, double *r_a,
                                  double *r_b, double *y_a, double *y_b, double *w_a, double *w_b, double *t, double *hist_dev,
                                  double *scal_dev, void *dot_work, void *work, int64_t first_iter, int iters, void *stream)
{
    const int64_t nrows = a.nrows;
    if (iters < 0 || first_iter < 1) return set_error(HPCLA_ERR_INVALID, "minres_iterations: negative count or first_iter < 1");
    if (nrows < 0 || a.nnz < 0) return set_error(HPCLA_ERR_INVALID, "minres_iterations: negative size");
    if (!hist_dev || !scal_dev || !dot_work || !work)
        return set_error(HPCLA_ERR_INVALID, "minres_iterations: null scalar / work buffer");
    if (nrows > 0 && (!x || !r_a || !r_b || !w_a || !w_b || !t || (dinv && (!y_a || !y_b))))
        return set_error(HPCLA_ERR_INVALID, "minres_iterations: null vector");
    if (misaligned16({x, r_a, r_b, w_a, w_b, t, dinv, dinv ? y_a : nullptr, dinv ? y_b : nullptr}))
        return set_error(HPCLA_ERR_INVALID, "minres_iterations: vectors must be 16-byte aligned");
    int64_t *state = solver_state(work, hpcla_minres_work_bytes());
    double *rbuf[2] = {r_a, r_b}, *wbuf[2] = {w_a, w_b};
    double *ybuf[2] = {dinv ? y_a : r_a, dinv ? y_b : r_b};
    for (int64_t j = first_iter; j < first_iter + iters; ++j) {
        const int cur = (int)((j - 1) & 1), nxt = (int)(j & 1);
        int rc = spmv_dist_dot(a, comm, ybuf[cur], nrows, t, scal_dev + MINRES_YT, dot_work, stream);
        if (rc) return rc;
        rc = hpcla_minres_r_f64(comm, scal_dev, t, rbuf[cur], dinv, rbuf[nxt], dinv ? ybuf[nxt] : nullptr, nrows, j, state,
                                hist_dev + 2 * j, work, stream);
        if (rc) return rc;
        rc = hpcla_minres_xw_f64(scal_dev, ybuf[cur], wbuf[cur], wbuf[nxt], x, nrows, j, state, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

HPCLA_API int hpcla_minres_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                              const int32_t *colval_split, const int16_t *cols16,
                                              const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows,
                                              int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                              const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, double *x,
                                              double *r_a, double *r_b, double *y_a, double *y_b, double *w_a, double *w_b,
                                              double *t, double *hist_dev, double *scal_dev, void *dot_work, void *work,
                                              int64_t first_iter, int iters, void *stream)
{
    return minres_iterations_impl<int32_t>({plan, rowptr, colval_split, cols16, patterns, nzval, nrows, nnz, index_base,
                                            interior_blocks, n_interior, boundary_blocks, n_boundary},
                                           comm, dinv, x, r_a, r_b, y_a, y_b, w_a, w_b, t, hist_dev, scal_dev, dot_work, work,
                                           first_iter, iters, stream);
}

HPCLA_API int hpcla_minres_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                              const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                              int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                              const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv, double *x,
                                              double *r_a, double *r_b, double *y_a, double *y_b, double *w_a, double *w_b,
                                              double *t, double *hist_dev, double *scal_dev, void *dot_work, void *work,
                                              int64_t first_iter, int iters, void *stream)
{
    return minres_iterations_impl<int64_t>({plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base,
                                            interior_blocks, n_interior, boundary_blocks, n_boundary},
                                           comm, dinv, x, r_a, r_b, y_a, y_b, w_a, w_b, t, hist_dev, scal_dev, dot_work, work,
                                           first_iter, iters, stream);
}

// ---- a chunk of gated GMRES(m) inner steps in ONE host call (the solver, hp.gmres) -----------------------------------
// Right-preconditioned restarted GMRES with twice-applied classical Gram-Schmidt, K = identity (dinv == NULL: the SpMV reads
// the basis column itself) or dinv .*.  Step k = first_iter .. first_iter + iters - 1 (1-based over the whole solve), column
// j = (k - 1) mod m, c = j + 1 (the gates and the bytes: csrc/vecops.hip):
//   1. w = A z                      hpcla_spmv_dist_* -- always executed, not gated, no dot partials
//   2. h1 = V^T w                   hpcla_gmres_dots_f64: ceil(c / 8) all-reduces of at most 8 sums
//   3. w = w - V h1                 hpcla_gmres_update_f64, first pass
//   4. h2 = V^T w                   the dots again
//   5. w = w - V h2, nn = w.w       hpcla_gmres_update_f64, second pass: one all-reduce [nn], the small step, gates D and C
//   6. V_{j+1} = w / col_c  [z]     hpcla_gmres_next_f64 while c < m
//   at c == m, every launch gated:  hpcla_gmres_solve_f64, hpcla_gmres_xupdate_f64 and the restart (w = A x, w = b - w, gate R,
//                                   V_0 = w / beta [z]) -- one more SpMV per cycle
// One rank: SpMV + 6 + 2 ceil(c / 8) launches per step.  N ranks: + 2 ceil(c / 8) + 1 window all-reduces and one 64-lane
// small-step launch.  hist_dev[2 k] = g[j+1]^2, the Givens estimate of sum r_k^2 (the true one at a gate R stop and at k = 0);
// hist_dev[2 k + 1] is not used (the layout is the other solvers' history of pairs).
template <typename I>
static int gmres_restart_impl(const SpmvBlock<I> &a, hpcla_comm_t *comm, const double *dinv, const double *b, const double *x,
                              double *V, double *w, double *z, double *small_dev, double *hist_dev, int64_t *state, void *work,
                              int restart, int64_t iter, void *stream)
{
    const int64_t nrows = a.nrows;
    int rc = spmv_dist(a, x, nrows, w, stream);
    if (rc) return rc;
    rc = hpcla_gmres_residual_f64(comm, b, w, nrows, iter, restart, small_dev, hist_dev + 2 * iter, state, work, stream);
    if (rc) return rc;
    const double *hn = small_dev + hpcla_gmres_small_offset(restart, 9);
    return hpcla_gmres_next_f64(w, hn, dinv, V, dinv ? z : nullptr, nrows, state, stream);
}

// The first half of the twice-applied classical Gram-Schmidt of w against c columns of V, shared with hp.eigsh and hp.svds:
// h1 = V^T w, w = w - V h1 (the first pass: no small step, no history), h2 = V^T w.  The caller's own update kernel ends it.
static int cgs2_first_half(hpcla_comm_t *comm, const double *V, int64_t ldv, int c, double *w, int64_t n, int64_t k, int m,
                           int64_t *state, double *h1, double *h2, void *work, void *stream)
{
    int rc = hpcla_gmres_dots_f64(comm, V, ldv, c, w, n, state, h1, work, stream);
    if (rc) return rc;
    rc = hpcla_gmres_update_f64(comm, V, ldv, c, h1, w, n, k, m, nullptr, nullptr, state, work, stream);
    if (rc) return rc;
    return hpcla_gmres_dots_f64(comm, V, ldv, c, w, n, state, h2, work, stream);
}

static int gmres_check(const char *who, int64_t nrows, int64_t nnz, int64_t ldv, int restart, const double *dinv, const double *b,
                       const double *x, const double *V, const double *w, const double *z, const double *small_dev,
                       const double *hist_dev, const void *work)
{
    if (nrows < 0 || nnz < 0) return set_error(HPCLA_ERR_INVALID, "%s: negative size", who);
    if (restart < 1 || restart > 64) return set_error(HPCLA_ERR_INVALID, "%s: restart must be in 1..64", who);
    if (ldv < nrows || (ldv & 1)) return set_error(HPCLA_ERR_INVALID, "%s: the pitch must be even and at least nrows", who);
    if (!small_dev || !hist_dev || !work) return set_error(HPCLA_ERR_INVALID, "%s: null small arrays / history / work", who);
    if (nrows > 0 && (!b || !x || !V || !w || (dinv && !z))) return set_error(HPCLA_ERR_INVALID, "%s: null vector", who);
    if (misaligned16({b, x, V, w, dinv, dinv ? z : nullptr}))
        return set_error(HPCLA_ERR_INVALID, "%s: vectors must be 16-byte aligned", who);
    return HPCLA_OK;
}

template <typename I>
static int gmres_iterations_impl(const SpmvBlock<I> &a, hpcla_comm_t *comm, const double *dinv, const double *b, double *x,
                                 double *V, int64_t ldv, double *w, double *z, double *small_dev, double *hist_dev, void *work,
                                 int restart, int64_t first_iter, int iters, void *stream)
{
    const int64_t nrows = a.nrows;
    if (iters < 0 || first_iter < 1) return set_error(HPCLA_ERR_INVALID, "gmres_iterations: negative count or first_iter < 1");
    if (int rc = gmres_check("gmres_iterations", nrows, a.nnz, ldv, restart, dinv, b, x, V, w, z, small_dev, hist_dev, work)) return rc;
    int64_t *state = solver_state(work, hpcla_gmres_work_bytes(restart));
    double *h1 = small_dev + hpcla_gmres_small_offset(restart, 4), *h2 = small_dev + hpcla_gmres_small_offset(restart, 5);
    double *y = small_dev + hpcla_gmres_small_offset(restart, 7), *hn = small_dev + hpcla_gmres_small_offset(restart, 9);
    for (int64_t k = first_iter; k < first_iter + iters; ++k) {
        const int j = (int)((k - 1) % restart), c = j + 1;
        const double *in = dinv ? z : V + (int64_t)j * ldv;
        int rc = spmv_dist(a, in, nrows, w, stream);
        if (rc) return rc;
        rc = cgs2_first_half(comm, V, ldv, c, w, nrows, k, restart, state, h1, h2, work, stream);
        if (rc) return rc;
        rc = hpcla_gmres_update_f64(comm, V, ldv, c, h2, w, nrows, k, restart, small_dev, hist_dev + 2 * k, state, work, stream);
        if (rc) return rc;
        if (c < restart) {
            rc = hpcla_gmres_next_f64(w, hn, dinv, V + (int64_t)c * ldv, dinv ? z : nullptr, nrows, state, stream);
            if (rc) return rc;
            continue;
        }
        rc = hpcla_gmres_solve_f64(c, restart, small_dev, state, stream);
        if (rc) return rc;
        rc = hpcla_gmres_xupdate_f64(V, ldv, c, y, dinv, x, nrows, state, stream);
        if (rc) return rc;
        rc = gmres_restart_impl<I>(a, comm, dinv, b, x, V, w, z, small_dev, hist_dev, state, work, restart, k, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

HPCLA_API int hpcla_gmres_iterations_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                             const int32_t *colval_split, const int16_t *cols16,
                                             const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows,
                                             int64_t nnz, int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                             const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv,
                                             const double *b, double *x, double *V, int64_t ldv, double *w, double *z,
                                             double *small_dev, double *hist_dev, void *work, int restart, int64_t first_iter,
                                             int iters, void *stream)
{
    return gmres_iterations_impl<int32_t>({plan, rowptr, colval_split, cols16, patterns, nzval, nrows, nnz, index_base,
                                           interior_blocks, n_interior, boundary_blocks, n_boundary},
                                          comm, dinv, b, x, V, ldv, w, z, small_dev, hist_dev, work, restart, first_iter, iters,
                                          stream);
}

HPCLA_API int hpcla_gmres_iterations_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                             const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                             int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                             const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv,
                                             const double *b, double *x, double *V, int64_t ldv, double *w, double *z,
                                             double *small_dev, double *hist_dev, void *work, int restart, int64_t first_iter,
                                             int iters, void *stream)
{
    return gmres_iterations_impl<int64_t>({plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base,
                                           interior_blocks, n_interior, boundary_blocks, n_boundary},
                                          comm, dinv, b, x, V, ldv, w, z, small_dev, hist_dev, work, restart, first_iter, iters,
                                          stream);
}

// The start of a cycle at iteration iter >= 0 on its own (the solver's setup from a given x0): w = A x, w = b - w, gate R,
// g = (beta, 0, ...), V_0 = w / beta [z = dinv .* V_0].  hist_dev[2 iter] receives w.w at iter = 0 and at a gate R stop.
template <typename I>
static int gmres_restart_checked(const SpmvBlock<I> &a, hpcla_comm_t *comm, const double *dinv, const double *b, const double *x,
                                 double *V, int64_t ldv, double *w, double *z, double *small_dev, double *hist_dev, void *work,
                                 int restart, int64_t iter, void *stream)
{
    if (iter < 0) return set_error(HPCLA_ERR_INVALID, "gmres_restart: negative iteration");
    if (int rc = gmres_check("gmres_restart", a.nrows, a.nnz, ldv, restart, dinv, b, x, V, w, z, small_dev, hist_dev, work)) return rc;
    int64_t *state = solver_state(work, hpcla_gmres_work_bytes(restart));
    return gmres_restart_impl<I>(a, comm, dinv, b, x, V, w, z, small_dev, hist_dev, state, work, restart, iter, stream);
}

HPCLA_API int hpcla_gmres_restart_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                          const int32_t *colval_split, const int16_t *cols16,
                                          const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows, int64_t nnz,
                                          int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                          const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv,
                                          const double *b, const double *x, double *V, int64_t ldv, double *w, double *z,
                                          double *small_dev, double *hist_dev, void *work, int restart, int64_t iter,
                                          void *stream)
{
    return gmres_restart_checked<int32_t>({plan, rowptr, colval_split, cols16, patterns, nzval, nrows, nnz, index_base,
                                           interior_blocks, n_interior, boundary_blocks, n_boundary},
                                          comm, dinv, b, x, V, ldv, w, z, small_dev, hist_dev, work, restart, iter, stream);
}

HPCLA_API int hpcla_gmres_restart_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                          const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                          int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                          const int32_t *boundary_blocks, int64_t n_boundary, const double *dinv,
                                          const double *b, const double *x, double *V, int64_t ldv, double *w, double *z,
                                          double *small_dev, double *hist_dev, void *work, int restart, int64_t iter,
                                          void *stream)
{
    return gmres_restart_checked<int64_t>({plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base,
                                           interior_blocks, n_interior, boundary_blocks, n_boundary},
                                          comm, dinv, b, x, V, ldv, w, z, small_dev, hist_dev, work, restart, iter, stream);
}

// ---- columns of a thick-restart Lanczos cycle in ONE host call (the eigensolver, hp.eigsh) ---------------------------------
// Full reorthogonalisation by twice-applied classical Gram-Schmidt on the GMRES kernels.  Column j = first_col ..
// first_col + count - 1 of a cycle of ncv columns, c = j + 1, step first_iter + (j - first_col) of the solve:
//   1. w = A V_j                    hpcla_spmv_dist_* -- always executed, not gated
//   2. h1 = V^T w                   hpcla_gmres_dots_f64
//   3. w = w - V h1                 hpcla_gmres_update_f64, first pass
//   4. h2 = V^T w                   the dots again
//   5. w = w - V h2, nn = w.w       hpcla_eigsh_update_f64: one all-reduce [nn], the Lanczos small step, gates N and I
//   6. V_{j+1} = w / hn             hpcla_gmres_next_f64, also at c == ncv: the basis has ncv + 1 columns
// One rank: SpMV + 6 + 2 ceil(c / 8) launches per step, no read-back.  The host reads the small buffer once per cycle.
template <typename I>
static int eigsh_steps_impl(const SpmvBlock<I> &a, hpcla_comm_t *comm, double *V, int64_t ldv, double *w, double *small_dev,
                            void *work, int ncv, int first_col, int count, int64_t first_iter, void *stream)
{
    const int64_t nrows = a.nrows;
    if (nrows < 0 || a.nnz < 0) return set_error(HPCLA_ERR_INVALID, "eigsh_steps: negative size");
    if (ncv < 1 || ncv > 64) return set_error(HPCLA_ERR_INVALID, "eigsh_steps: ncv must be in 1..64");
    if (first_col < 0 || count < 0 || first_col + count > ncv || first_iter < 1)
        return set_error(HPCLA_ERR_INVALID, "eigsh_steps: columns outside 0..ncv-1 or first_iter < 1");
    if (ldv < nrows || (ldv & 1)) return set_error(HPCLA_ERR_INVALID, "eigsh_steps: the pitch must be even and at least nrows");
    if (!small_dev || !work) return set_error(HPCLA_ERR_INVALID, "eigsh_steps: null small arrays / work");
    if (nrows > 0 && (!V || !w)) return set_error(HPCLA_ERR_INVALID, "eigsh_steps: null vector");
    if (misaligned16({V, w})) return set_error(HPCLA_ERR_INVALID, "eigsh_steps: vectors must be 16-byte aligned");
    int64_t *state = solver_state(work, hpcla_gmres_work_bytes(ncv));
    double *h1 = small_dev + hpcla_eigsh_small_offset(ncv, 2), *h2 = small_dev + hpcla_eigsh_small_offset(ncv, 3);
    double *hn = small_dev + hpcla_eigsh_small_offset(ncv, 5);
    for (int j = first_col; j < first_col + count; ++j) {
        const int c = j + 1;
        const int64_t k = first_iter + (j - first_col);
        int rc = spmv_dist(a, V + (int64_t)j * ldv, nrows, w, stream);
        if (rc) return rc;
        rc = cgs2_first_half(comm, V, ldv, c, w, nrows, k, ncv, state, h1, h2, work, stream);
        if (rc) return rc;
        rc = hpcla_eigsh_update_f64(comm, V, ldv, c, h2, w, nrows, k, ncv, small_dev, state, work, stream);
        if (rc) return rc;
        rc = hpcla_gmres_next_f64(w, hn, nullptr, V + (int64_t)c * ldv, nullptr, nrows, state, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

HPCLA_API int hpcla_eigsh_steps_f64_i32(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int32_t *rowptr,
                                        const int32_t *colval_split, const int16_t *cols16, const hpcla_block_patterns_t *patterns,
                                        const double *nzval, int64_t nrows, int64_t nnz, int index_base,
                                        const int32_t *interior_blocks, int64_t n_interior, const int32_t *boundary_blocks,
                                        int64_t n_boundary, double *V, int64_t ldv, double *w, double *small_dev, void *work,
                                        int ncv, int first_col, int count, int64_t first_iter, void *stream)
{
    return eigsh_steps_impl<int32_t>({plan, rowptr, colval_split, cols16, patterns, nzval, nrows, nnz, index_base, interior_blocks,
                                      n_interior, boundary_blocks, n_boundary},
                                     comm, V, ldv, w, small_dev, work, ncv, first_col, count, first_iter, stream);
}

HPCLA_API int hpcla_eigsh_steps_f64_i64(hpcla_halo_plan_t *plan, hpcla_comm_t *comm, const int64_t *rowptr,
                                        const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                        int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                        const int32_t *boundary_blocks, int64_t n_boundary, double *V, int64_t ldv, double *w,
                                        double *small_dev, void *work, int ncv, int first_col, int count, int64_t first_iter,
                                        void *stream)
{
    return eigsh_steps_impl<int64_t>({plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base, interior_blocks,
                                      n_interior, boundary_blocks, n_boundary},
                                     comm, V, ldv, w, small_dev, work, ncv, first_col, count, first_iter, stream);
}

// ---- columns of a thick-restart Golub-Kahan cycle in ONE host call (the truncated SVD, hp.svds) ------------------------------
// A of any shape nrows x nrows_t, At its materialised transpose (a matrix and a plan of its own, as for hpcla_lsqr_iterations_*).
// Two bases: U (ncv columns of nrows doubles at the even pitch ldu) and V (ncv + 1 columns of nrows_t doubles at ldv); full
// two-sided reorthogonalisation by twice-applied classical Gram-Schmidt on the GMRES kernels.  Column j = first_col ..
// first_col + count - 1 of a cycle of ncv columns, step first_iter + (j - first_col) of the solve:
//   1. u = A V_j                    hpcla_spmv_dist_* on A's plan -- always executed, not gated
//   2. g1 = U^T u; u = u - U g1; g2 = U^T u          gmres_dots, gmres_update (first pass), gmres_dots over j columns (none at j = 0)
//   3. u = u - U g2, aa = u.u       hpcla_svds_update_f64, side 0: one all-reduce [aa], B's column j and alpha_j, gates N and Z
//   4. U_j = u / alpha_j            hpcla_gmres_next_f64
//   5. v = At U_j                   the SpMV on At's plan -- always executed
//   6. h1 = V^T v; v = v - V h1; h2 = V^T v          the same three over j + 1 columns
//   7. v = v - V h2, bb = v.v       hpcla_svds_update_f64, side 1: one all-reduce [bb], beta_j, gates N' and Z'
//   8. V_{j+1} = v / beta_j         hpcla_gmres_next_f64, also at j + 1 == ncv: the right basis has ncv + 1 columns
// One rank: 2 SpMV + 12 + 2 ceil(j / 8) + 2 ceil((j + 1) / 8) launches per step (11 at j = 0), no read-back.  The host reads the small buffer
// once per cycle.
template <typename I>
static int svds_steps_impl(hpcla_comm_t *comm, const SpmvBlock<I> &a, const SpmvBlock<I> &at, double *U, int64_t ldu, double *V,
                           int64_t ldv, double *u, double *v, double *small_dev, void *work, int ncv, int first_col, int count,
                           int64_t first_iter, void *stream)
{
    const int64_t nrows = a.nrows, nrows_t = at.nrows;
    if (nrows < 0 || a.nnz < 0 || nrows_t < 0 || at.nnz < 0) return set_error(HPCLA_ERR_INVALID, "svds_steps: negative size");
    if (ncv < 1 || ncv > 64) return set_error(HPCLA_ERR_INVALID, "svds_steps: ncv must be in 1..64");
    if (first_col < 0 || count < 0 || first_col + count > ncv || first_iter < 1)
        return set_error(HPCLA_ERR_INVALID, "svds_steps: columns outside 0..ncv-1 or first_iter < 1");
    if (ldu < nrows || (ldu & 1) || ldv < nrows_t || (ldv & 1))
        return set_error(HPCLA_ERR_INVALID, "svds_steps: both pitches must be even and at least the local length");
    if (!small_dev || !work) return set_error(HPCLA_ERR_INVALID, "svds_steps: null small arrays / work");
    if ((nrows > 0 && (!U || !u)) || (nrows_t > 0 && (!V || !v))) return set_error(HPCLA_ERR_INVALID, "svds_steps: null vector");
    if (misaligned16({U, V, u, v})) return set_error(HPCLA_ERR_INVALID, "svds_steps: vectors must be 16-byte aligned");
    int64_t *state = solver_state(work, hpcla_gmres_work_bytes(ncv));
    double *g1 =small_dev + hpcla_svds_small_offset(ncv, 2), *g2 = small_dev + hpcla_svds_small_offset(ncv, 3);
    double *h1 = small_dev + hpcla_svds_small_offset(ncv, 4), *h2 = small_dev + hpcla_svds_small_offset(ncv, 5);
    double *dv = small_dev + hpcla_svds_small_offset(ncv, 8);
    for (int j = first_col; j < first_col + count; ++j) {
        const int64_t k = first_iter + (j - first_col);
        double *Uj = U + (int64_t)j * ldu;
        int rc = spmv_dist(a, V + (int64_t)j * ldv, nrows_t, u, stream);
        if (rc) return rc;
        if (j > 0) {
            rc = cgs2_first_half(comm, U, ldu, j, u, nrows, k, ncv, state, g1, g2, work, stream);
            if (rc) return rc;
        }
        rc = hpcla_svds_update_f64(comm, U, ldu, j, g2, u, nrows, k, ncv, 0, small_dev, state, work, stream);
        if (rc) return rc;
        rc = hpcla_gmres_next_f64(u, dv, nullptr, Uj, nullptr, nrows, state, stream);
        if (rc) return rc;
        rc = spmv_dist(at, Uj, nrows, v, stream);
        if (rc) return rc;
        rc = cgs2_first_half(comm, V, ldv, j + 1, v, nrows_t, k, ncv, state, h1, h2, work, stream);
        if (rc) return rc;
        rc = hpcla_svds_update_f64(comm, V, ldv, j + 1, h2, v, nrows_t, k, ncv, 1, small_dev, state, work, stream);
        if (rc) return rc;
        rc = hpcla_gmres_next_f64(v, dv, nullptr, V + (int64_t)(j + 1) * ldv, nullptr, nrows_t, state, stream);
        if (rc) return rc;
    }
    return HPCLA_OK;
}

HPCLA_API int hpcla_svds_steps_f64_i32(hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int32_t *rowptr,
                                       const int32_t *colval_split, const int16_t *cols16,
                                       const hpcla_block_patterns_t *patterns, const double *nzval, int64_t nrows, int64_t nnz,
                                       int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                       const int32_t *boundary_blocks, int64_t n_boundary, hpcla_halo_plan_t *plan_t,
                                       const int32_t *rowptr_t, const int32_t *colval_split_t, const int16_t *cols16_t,
                                       const hpcla_block_patterns_t *patterns_t, const double *nzval_t, int64_t nrows_t,
                                       int64_t nnz_t, int index_base_t, const int32_t *interior_blocks_t, int64_t n_interior_t,
                                       const int32_t *boundary_blocks_t, int64_t n_boundary_t, double *U, int64_t ldu, double *V,
                                       int64_t ldv, double *u, double *v, double *small_dev, void *work, int ncv, int first_col,
                                       int count, int64_t first_iter, void *stream)
{
    return svds_steps_impl<int32_t>(comm,
                                    {plan, rowptr, colval_split, cols16, patterns, nzval, nrows, nnz, index_base, interior_blocks,
                                     n_interior, boundary_blocks, n_boundary},
                                    {plan_t, rowptr_t, colval_split_t, cols16_t, patterns_t, nzval_t, nrows_t, nnz_t, index_base_t,
                                     interior_blocks_t, n_interior_t, boundary_blocks_t, n_boundary_t},
                                    U, ldu, V, ldv, u, v, small_dev, work, ncv, first_col, count, first_iter, stream);
}

HPCLA_API int hpcla_svds_steps_f64_i64(hpcla_comm_t *comm, hpcla_halo_plan_t *plan, const int64_t *rowptr,
                                       const int64_t *colval_split, const double *nzval, int64_t nrows, int64_t nnz,
                                       int index_base, const int32_t *interior_blocks, int64_t n_interior,
                                       const int32_t *boundary_blocks, int64_t n_boundary, hpcla_halo_plan_t *plan_t,
                                       const int64_t *rowptr_t, const int64_t *colval_split_t, const double *nzval_t,
                                       int64_t nrows_t, int64_t nnz_t, int index_base_t, const int32_t *interior_blocks_t,
                                       int64_t n_interior_t, const int32_t *boundary_blocks_t, int64_t n_boundary_t, double *U,
                                       int64_t ldu, double *V, int64_t ldv, double *u, double *v, double *small_dev, void *work,
                                       int ncv, int first_col, int count, int64_t first_iter, void *stream)
{
    return svds_steps_impl<int64_t>(comm,
                                    {plan, rowptr, colval_split, nullptr, nullptr, nzval, nrows, nnz, index_base, interior_blocks,
                                     n_interior, boundary_blocks, n_boundary},
                                    {plan_t, rowptr_t, colval_split_t, nullptr, nullptr, nzval_t, nrows_t, nnz_t, index_base_t,
                                     interior_blocks_t, n_interior_t, boundary_blocks_t, n_boundary_t},
                                    U, ldu, V, ldv, u, v, small_dev, work, ncv, first_col, count, first_iter, stream);
}
