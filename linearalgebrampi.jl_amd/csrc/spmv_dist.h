// spmv_dist.h -- the distributed product as the solver loops see it: one matrix as one SpmvBlock, y = A x and its fused
// x.y (defined in comm.hip, called from solvers.hip).  Library-internal.
#pragma once
#include "common.h"

namespace hpcla {

template <typename I>
struct SpmvBlock {                                                  // the plan and CSR arguments of one matrix
    hpcla_halo_plan_t *plan;
    const I *rowptr, *colval;
    const int16_t *cols16;
    const hpcla_block_patterns *patterns;
    const double *nzval;
    int64_t nrows, nnz;
    int index_base;
    const int32_t *interior;
    int64_t n_interior;
    const int32_t *boundary;
    int64_t n_boundary;
};

// the last 32 bytes of a solver's `work`: its device-resident state words
static inline int64_t *solver_state(void *work, int64_t work_bytes)
{
    return reinterpret_cast<int64_t *>(static_cast<char *>(work) + work_bytes) - 4;
}

// y = A x: the launches of hpcla_spmv_dist_* (cols16 / patterns null: those of the plain Int32 / Int64 entries)
int spmv_dist(const SpmvBlock<int32_t> &m, const double *x, int64_t n_own, double *y, void *stream);
int spmv_dist(const SpmvBlock<int64_t> &m, const double *x, int64_t n_own, double *y, void *stream);
// y = A x and *dot_out_dev = x.y, all-reduced over comm: the launches of hpcla_spmv_dist_dot_*
int spmv_dist_dot(const SpmvBlock<int32_t> &m, hpcla_comm_t *comm, const double *x, int64_t n_own, double *y,
                  double *dot_out_dev, void *work, void *stream);
int spmv_dist_dot(const SpmvBlock<int64_t> &m, hpcla_comm_t *comm, const double *x, int64_t n_own, double *y,
                  double *dot_out_dev, void *work, void *stream);

}  // namespace hpcla
