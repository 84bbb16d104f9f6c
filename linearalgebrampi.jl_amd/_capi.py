"""ctypes binding of libhpcla_rocm.so (include/hpcla_rocm.h).

This is the Python twin of the ``@ccall`` stubs in INTEGRATION.md: same entry points, same
status convention (`status == 0 || error(...)`, cf. ext/HPCLinearAlgebraCUDAExt.jl:248-251).
There is no fallback: if the shared library is missing or fails to load, importing the package's
device layer raises.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhpcla_rocm.so")

OK = 0
LAYOUT_ROW = 0
LAYOUT_COL = 1
UNIQUE_ID_BYTES = 128
WINDOW_DESC_BYTES = 128
WINDOW_TABLE_ROWS = 4
COMM_NO_RCCL = 1
HALO_SINGLE_BUFFER = 1
BLOCK_PATTERNS_WEAK_HASH = 1


class HPCLAError(RuntimeError):
    def __init__(self, fn: str, status: int, text: str):
        super().__init__(f"{fn} failed with status {status}: {text}")
        self.status = status


_lib = None

_i32 = ctypes.c_int
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64
_f64 = ctypes.c_double
_f32 = ctypes.c_float
_vp = ctypes.c_void_p

# name -> argtypes ; every function returns int status unless listed in _RESTYPES
_SIGNATURES = {
    "hpcla_version": [],
    "hpcla_last_error": [],
    "hpcla_device_count": [_vp],
    "hpcla_set_device": [_i32],
    "hpcla_device_info": [_i32, _vp, _vp, _i32],
    "hpcla_spmv_csr_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp],
    "hpcla_spmv_csr_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp],
    "hpcla_spmv_split_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp],
    "hpcla_spmv_split_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp],
    "hpcla_spmv_rows_per_block": [],
    "hpcla_spmv_longrows_work_bytes": [_i64],
    "hpcla_spmv_longrows_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _vp, _vp],
    "hpcla_spmv_longrows_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _vp, _vp],
    "hpcla_spmv_block_order_hint": [_vp, _i32],
    "hpcla_block_order_decide": [_vp, _i32, _i32, _vp],
    "hpcla_set_spmv_sweep": [_i32],
    "hpcla_spmv_last_sweep": [_vp],
    "hpcla_spmv_tune_block_order_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp],
    "hpcla_spmv_tune_block_order_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp],
    "hpcla_spmv_tune_block_order_cols16_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i64, _i64, _vp, _vp],
    "hpcla_cols16_padded_len": [_i64],
    "hpcla_cols16_encode_i32": [_vp, _vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp],
    "hpcla_spmv_cols16_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp],
    "hpcla_block_patterns_create_i32": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp],
    "hpcla_block_patterns_destroy": [_vp],
    "hpcla_block_patterns_info": [_vp, _vp, _vp, _vp, _vp],
    "hpcla_spmv_patterns_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp],
    "hpcla_spmv_tune_block_order_patterns_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i64, _i64, _vp, _vp],
    "hpcla_spmm_rows_per_block": [],
    "hpcla_spmm_runs_desc_bytes": [_i64],
    "hpcla_spmm_runs_build_i32": [_vp, _vp, _i64, _i64, _i32, _i64, _vp, _vp, _vp],
    "hpcla_spmm_runs_build_i64": [_vp, _vp, _i64, _i64, _i32, _i64, _vp, _vp, _vp],
    "hpcla_spmm_banded_blocks_i32": [_vp, _vp, _i64, _i64, _i32, _i64, _i32, _vp, _vp],
    "hpcla_spmm_banded_blocks_i64": [_vp, _vp, _i64, _i64, _i32, _i64, _i32, _vp, _vp],
    "hpcla_spmm_runs_k16_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _vp],
    "hpcla_spmm_runs_k16_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _vp],
    "hpcla_spmm_runs_colmajor_k16_f64_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp],
    "hpcla_spmm_runs_colmajor_k16_f64_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp],
    "hpcla_spmm_runs_colmajor_tune_block_order_f64_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp],
    "hpcla_spmm_runs_colmajor_tune_block_order_f64_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp],
    "hpcla_spmm_block_order_hint": [_vp, _i32],
    "hpcla_spmm_tune_block_order_f64_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32,
                                            _vp, _i64, _vp, _vp],
    "hpcla_spmm_tune_block_order_f64_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32,
                                            _vp, _i64, _vp, _vp],
    "hpcla_remap_i32": [_vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_remap_i64": [_vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_remap_i64_to_i32": [_vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_narrow_i64_to_i32": [_vp, _vp, _i64, _vp, _vp],
    "hpcla_classify_blocks_i32": [_vp, _vp, _i64, _i32, _i64, _i32, _vp, _vp],
    "hpcla_classify_blocks_i64": [_vp, _vp, _i64, _i32, _i64, _i32, _vp, _vp],
    "hpcla_spmm_csr_f64_i32": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i32, _i32, _vp],
    "hpcla_spmm_csr_f64_i64": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i32, _i32, _vp],
    "hpcla_spmm_split_f64_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_spmm_split_f64_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_spmm_split_ccol_f64_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_spmm_split_ccol_f64_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_spmm_split_colmajor_f64_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_spmm_split_colmajor_f64_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_halo_begin_strided_f64": [_vp, _vp, _i64, _i64, _vp, _vp],
    "hpcla_spmm_panel_f64_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp],
    "hpcla_spmm_panel_f64_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp],
    "hpcla_transpose_f64": [_vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _vp],
    "hpcla_gather_f64_i32": [_vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_gather_f64_i64": [_vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_comm_get_unique_id": [_vp],
    "hpcla_comm_init_rank": [_vp, _vp, _i32, _i32],
    "hpcla_comm_init_rank_ex": [_vp, _vp, _i32, _i32, _i32],
    "hpcla_comm_window_export": [_vp, _vp],
    "hpcla_comm_window_attach": [_vp, _vp],
    "hpcla_comm_status": [_vp, _vp],
    "hpcla_comm_window_selftest": [_vp, _f64, _vp],
    "hpcla_comm_window_detach": [_vp],
    "hpcla_halo_plan_detach": [_vp],
    "hpcla_device_identity": [_i32, _vp],
    "hpcla_halo_plan_export": [_vp, _vp, _vp],
    "hpcla_halo_plan_attach": [_vp, _vp, _vp],
    "hpcla_halo_status": [_vp, _vp],
    "hpcla_halo_plan_probe": [_vp, _i64, _vp, _vp, _i64, _vp, _vp],
    "hpcla_set_halo_mode": [_i32],
    "hpcla_comm_rank": [_vp, _vp],
    "hpcla_comm_size": [_vp, _vp],
    "hpcla_comm_destroy": [_vp],
    "hpcla_allreduce_f64": [_vp, _vp, _i64, _i32, _vp],
    "hpcla_exchange_ranges_f64": [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp],
    "hpcla_halo_plan_create": [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32],
    "hpcla_halo_plan_create_ex": [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32],
    "hpcla_halo_plan_chain": [_vp, _vp],
    "hpcla_halo_plan_destroy": [_vp],
    "hpcla_halo_ghost_ptr": [_vp, _vp, _vp],
    "hpcla_halo_begin": [_vp, _vp, _vp],
    "hpcla_halo_end": [_vp, _vp],
    "hpcla_spmv_dist_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp],
    "hpcla_spmv_dist_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp],
    "hpcla_spmv_dist_cols16_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp],
    "hpcla_spmv_dist_dot_cols16_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                           _vp, _vp, _vp],
    "hpcla_spmv_dist_patterns_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp],
    "hpcla_spmv_dist_dot_patterns_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp,
                                             _i64, _vp, _vp, _vp],
    "hpcla_spmv_dot_work_bytes": [_i64],
    "hpcla_spmv_dist_dot_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp],
    "hpcla_spmv_dist_dot_f64_i64": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp],
    "hpcla_cg_update_f64": [_vp, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_cg_residual_f64": [_vp, _f64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_cg_direction_f64": [_f64, _vp, _vp, _f64, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "hpcla_cg_iterations_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _i32, _vp],
    "hpcla_cg_iterations_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _i32, _vp],
    # the converging solver (hp.cg): gated, diagonally preconditioned iterations
    "hpcla_pcg_work_bytes": [],
    "hpcla_pcg_residual_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_pcg_direction_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "hpcla_pcg_iterations_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_pcg_iterations_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    # factorised sparse approximate inverse (hp.fsai, csrc/fsai.hip): G's structure, its values; the chunk of CG iterations
    # with M = Gt G (the plan / CSR block three times: A, G, Gt)
    "hpcla_fsai_work_bytes": [_i64],
    "hpcla_fsai_count_f64_i32": [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_fsai_count_f64_i64": [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_fsai_factor_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp],
    "hpcla_fsai_factor_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp, _vp],
    # fine-grained ILU(0) (hp.ilu0, csrc/ilu.hip): the owned block's CSR, the factor sweeps, the triangular sweeps of an application
    "hpcla_ilu_work_bytes": [_i64],
    "hpcla_ilu_count_f64_i32": [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_ilu_count_f64_i64": [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_ilu_fill_f64_i32": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hpcla_ilu_fill_f64_i64": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hpcla_ilu_gather_f64": [_vp, _vp, _i64, _vp, _vp],
    "hpcla_ilu_init_f64": [_vp, _vp, _vp, _vp, _i64, _vp, _vp],
    "hpcla_ilu_sweep_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "hpcla_ilu_pivots_f64": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_ilu_trisweep_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp],
    "hpcla_ilu_apply_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp],
    "hpcla_pcg_fsai_iterations_f64_i32": [_vp,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_pcg_fsai_iterations_f64_i64": [_vp,
                                          _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                          _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                          _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    # smoothed-aggregation multigrid (hp.amg, csrc/amg.hip): a level's weights, strength graph, aggregation and prolongator
    # values; the cycle's two fused smoother updates
    "hpcla_amg_work_bytes": [_i64],
    "hpcla_amg_round_blocks": [_i64],
    "hpcla_amg_weights_f64_i32": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_amg_weights_f64_i64": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_amg_smoother_f64": [_f64, _vp, _vp, _i64, _vp],
    "hpcla_amg_strength_count_f64_i32": [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _f64, _vp, _vp, _vp, _vp],
    "hpcla_amg_strength_count_f64_i64": [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _f64, _vp, _vp, _vp, _vp],
    "hpcla_amg_strength_fill_f64_i32": [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _f64, _vp, _vp, _vp],
    "hpcla_amg_strength_fill_f64_i64": [_vp, _vp, _vp, _vp, _i64, _i64, _i32, _f64, _vp, _vp, _vp],
    "hpcla_amg_mis_init": [_i64, _i64, _vp, _vp, _vp],
    "hpcla_amg_mis_round": [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hpcla_amg_join": [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hpcla_amg_aggregate_ids": [_vp, _vp, _i64, _i64, _vp, _vp],
    "hpcla_amg_prolongator_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp],
    "hpcla_amg_prolongator_f64_i64": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp],
    "hpcla_amg_symmetrise_count": [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "hpcla_amg_symmetrise_fill": [_vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "hpcla_amg_restrictor_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp],
    "hpcla_amg_restrictor_f64_i64": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp],
    "hpcla_amg_fit_f64": [_vp, _i64, _i32, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_amg_prolongator_b_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp],
    "hpcla_amg_prolongator_b_f64_i64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp],
    "hpcla_amg_restrictor_b_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp, _vp],
    "hpcla_amg_restrictor_b_f64_i64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _i64, _i32, _vp, _vp],
    "hpcla_amg_presmooth_f64": [_vp, _vp, _vp, _i64, _vp],
    "hpcla_amg_postsmooth_f64": [_vp, _vp, _vp, _vp, _i64, _vp],
    # BiCGStab for nonsymmetric A (hp.bicgstab): the gated steps and the chunk of iterations
    "hpcla_bicgstab_work_bytes": [],
    "hpcla_bicg_dot_f64": [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    "hpcla_bicg_s_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "hpcla_bicg_tts_f64": [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_bicg_xr_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_bicg_p_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "hpcla_bicgstab_iterations_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_bicgstab_iterations_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    # LSQR for rectangular A (hp.lsqr): the gated steps and the chunk of iterations (the plan / CSR block twice: A, then At)
    "hpcla_lsqr_work_bytes": [],
    "hpcla_lsqr_u_f64": [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp],
    "hpcla_lsqr_v_f64": [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_lsqr_xw_f64": [_vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "hpcla_lsqr_iterations_f64_i32": [_vp,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_lsqr_iterations_f64_i64": [_vp,
                                      _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                      _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    # MINRES for symmetric indefinite A (hp.minres): the gated steps and the chunk of iterations
    "hpcla_minres_work_bytes": [],
    "hpcla_minres_r_f64": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_minres_xw_f64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp],
    "hpcla_minres_iterations_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_minres_iterations_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    # restarted GMRES (hp.gmres): the gated steps, the chunk of inner steps, the start and the finish of a cycle
    "hpcla_gmres_work_bytes": [_i32],
    "hpcla_gmres_small_offset": [_i32, _i32],
    "hpcla_gmres_dots_f64": [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _vp],
    "hpcla_gmres_update_f64": [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp],
    "hpcla_gmres_next_f64": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp],
    "hpcla_gmres_solve_f64": [_i32, _i32, _vp, _vp, _vp],
    "hpcla_gmres_xupdate_f64": [_vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp],
    "hpcla_gmres_residual_f64": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp],
    "hpcla_gmres_finish_f64": [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp],
    "hpcla_gmres_iterations_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                       _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp],
    "hpcla_gmres_iterations_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                       _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp],
    "hpcla_gmres_restart_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                    _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _vp],
    "hpcla_gmres_restart_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp,
                                    _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _vp],
    # thick-restart Lanczos (hp.eigsh): the Lanczos second pass, the columns of a cycle, the restart's rotate (csrc/eigsh.hip)
    "hpcla_eigsh_small_offset": [_i32, _i32],
    "hpcla_eigsh_update_f64": [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_eigsh_rotate_f64": [_vp, _i64, _i32, _i32, _vp, _i32, _vp, _i64, _i64, _i64, _vp],
    "hpcla_eigsh_steps_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp,
                                  _vp, _vp, _i32, _i32, _i32, _i64, _vp],
    "hpcla_eigsh_steps_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp,
                                  _vp, _vp, _i32, _i32, _i32, _i64, _vp],
    # thick-restart Golub-Kahan bidiagonalisation (hp.svds): the second pass of either side, the columns of a cycle
    "hpcla_svds_small_offset": [_i32, _i32],
    "hpcla_svds_update_f64": [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp],
    "hpcla_svds_steps_f64_i32": [_vp,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                 _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp],
    "hpcla_svds_steps_f64_i64": [_vp,
                                 _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                 _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64,
                                 _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _vp],
    # the block eigensolver (hp.lobpcg): the residual block with its column norms, the in-place combine (csrc/lobpcg.hip)
    "hpcla_lobpcg_chunk_rows": [_i64],
    "hpcla_lobpcg_work_bytes": [_i64, _i32],
    "hpcla_lobpcg_residual_f64": [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _vp],
    "hpcla_lobpcg_combine_f64": [_vp, _i64, _vp, _i64, _vp, _i32, _i32, _i64, _vp],
    # the same for the pencil A x = lambda B x: three sums per column, B W of a diagonal B
    "hpcla_lobpcg_gen_work_bytes": [_i64, _i32],
    "hpcla_lobpcg_residual_gen_f64": [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp,
                                      _vp],
    # tall-skinny Householder QR (hp.qr, hp.lstsq): the tree's constants, its workspace, the factorisation (csrc/qr.hip)
    "hpcla_qr_panel_rows": [],
    "hpcla_qr_fan": [_i32],
    "hpcla_qr_work_bytes": [_i64, _i32, _i32, _i32],
    "hpcla_qr_f64": [_vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp],
    "hpcla_colspace_work_bytes": [_i64],
    "hpcla_compress_columns_i32": [_vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp],
    "hpcla_compress_columns_i64": [_vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp],
    # range indexing of a sparse matrix (csrc/submatrix.hip)
    "hpcla_submatrix_work_bytes": [_i64, _i64],
    "hpcla_submatrix_scan_chunk": [],
    "hpcla_submatrix_structure_i32": [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hpcla_submatrix_structure_i64": [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "hpcla_submatrix_fill_i32": [_i32, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_submatrix_fill_i64": [_i32, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_submatrix_values_i32": [_i32, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _vp],
    "hpcla_submatrix_values_i64": [_i32, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _vp],
    "hpcla_sparse_column_i32": [_i32, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp],
    "hpcla_sparse_column_i64": [_i32, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _vp],
    "hpcla_sparse_diag_f64_i32": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _vp],
    "hpcla_sparse_diag_f64_i64": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _i64, _i64, _i32, _vp, _vp],
    # COO assembly with a reusable structure (hp.assembly_plan, csrc/assemble.hip)
    "hpcla_assemble_chunk": [],
    "hpcla_assemble_run": [],
    "hpcla_assemble_pass": [],
    "hpcla_assemble_work_bytes": [_i64],
    "hpcla_assemble_values_work_bytes": [_i64],
    "hpcla_assemble_keys": [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp],
    "hpcla_assemble_segments_i32": [_vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "hpcla_assemble_segments_i64": [_vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "hpcla_assemble_row_starts_i32": [_vp, _i64, _i64, _i64, _i32, _vp, _vp],
    "hpcla_assemble_row_starts_i64": [_vp, _i64, _i64, _i64, _i32, _vp, _vp],
    "hpcla_assemble_columns": [_vp, _i64, _i64, _i32, _vp, _vp],
    "hpcla_assemble_values_f64_i32": [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp],
    "hpcla_assemble_values_f64_i64": [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp],
    # index-set selection (hp.select, hp.take, hp.put_, csrc/select.hip)
    "hpcla_select_short_cap": [],
    "hpcla_select_tile": [],
    "hpcla_select_work_bytes": [_i64, _i64, _i64],
    "hpcla_select_structure_i32": [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp],
    "hpcla_select_structure_i64": [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp],
    "hpcla_select_fill_i32": [_i32, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp],
    "hpcla_select_fill_i64": [_i32, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp],
    "hpcla_gather_b32_i64": [_vp, _vp, _vp, _i64, _i64, _i32, _vp],
    "hpcla_select_take_f64_i32": [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp],
    "hpcla_select_take_f64_i64": [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp],
    "hpcla_select_put_f64_i32": [_vp, _i64, _vp, _vp, _i64, _i32, _vp],
    "hpcla_select_put_f64_i64": [_vp, _i64, _vp, _vp, _i64, _i32, _vp],
    # reverse Cuthill-McKee ordering and the bandwidth (hp.rcm, hp.bandwidth, csrc/rcm.hip)
    "hpcla_rcm_frontier_cap": [],
    "hpcla_rcm_candidate_cap": [],
    "hpcla_rcm_work_bytes": [_i64],
    "hpcla_rcm_graph_count_i32": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_rcm_graph_count_i64": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "hpcla_rcm_graph_fill_i32": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp],
    "hpcla_rcm_graph_fill_i64": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp],
    "hpcla_rcm_degrees": [_vp, _vp, _i64, _i32, _vp, _vp],
    "hpcla_rcm_init": [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "hpcla_rcm_narrow": [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp],
    "hpcla_rcm_expand": [_vp, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_rcm_keys": [_vp, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_rcm_number": [_vp, _i64, _i64, _vp, _i64, _vp, _vp],
    "hpcla_rcm_finish": [_vp, _i64, _i64, _vp, _vp, _vp],
    "hpcla_rcm_graph_bandwidth": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_bandwidth_i32": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp],
    "hpcla_bandwidth_i64": [_vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp],
    "hpcla_digest_i32": [_vp, _i64, _vp, _vp],
    "hpcla_digest_i64": [_vp, _i64, _vp, _vp],
    "hpcla_poisson2d_nnz": [_i64, _i64, _i64, _i64],
    "hpcla_gen_poisson2d": [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_poisson3d_nnz": [_i64, _i64, _i64, _i64, _i64],
    "hpcla_gen_poisson3d": [_i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_gemv_rowmajor_f64": [_vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp],
    "hpcla_gemv_t_work_bytes": [_i64, _i64],
    "hpcla_gemv_t_rowmajor_f64": [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp],
    "hpcla_gram_work_bytes": [_i64, _i64, _i64],
    "hpcla_gram_f64": [_vp, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i64, _vp, _vp, _vp],
    "hpcla_gram_f32": [_vp, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i64, _vp, _vp, _vp],
    "hpcla_spmm_t_struct_work_bytes": [_i64, _i64, _i32],
    "hpcla_spmm_t_struct_i32": [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp],
    "hpcla_spmm_t_struct_i64": [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp],
    "hpcla_spmm_t_f64_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _vp],
    "hpcla_spmm_t_f64_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _i64, _vp, _i64, _i32, _vp],
    "hpcla_spmm_t_accumulate_f64": [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp],
    "hpcla_spgemm_bin_cap": [_i32],
    "hpcla_spgemm_ub_i32": [_vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "hpcla_spgemm_ub_i64": [_vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "hpcla_spgemm_numeric_i32": [_i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "hpcla_spgemm_numeric_i64": [_i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "hpcla_spgemm_compact": [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "hpcla_spgemm_numeric_mapped_f64": [_vp, _i32, _vp, _vp, _vp, _vp, _i64, _vp],
    "hpcla_packed_create_i32": [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp],
    "hpcla_packed_destroy": [_vp],
    "hpcla_packed_info": [_vp, _vp, _vp],
    "hpcla_spmv_packed_f64_i32": [_vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp],
    "hpcla_spmv_dist_packed_f64_i32": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64,
                                       _vp, _i64, _vp, _vp, _vp],
    "hpcla_reduce_work_bytes": [],
    "hpcla_dot_f64": [_vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_nrm2sq_f64": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_asum_f64": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_amax_f64": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_maxval_f64": [_vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "hpcla_sum_f64": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_prod_f64": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_powsum_f64": [_vp, _vp, _i64, _f64, _vp, _vp, _vp],
    "hpcla_axpy_f64": [_f64, _vp, _vp, _vp, _vp, _i64, _vp],
    "hpcla_xpay_f64": [_vp, _f64, _vp, _vp, _vp, _i64, _vp],
    "hpcla_scale_f64": [_f64, _vp, _vp, _i64, _vp],
    "hpcla_divide_f64": [_vp, _f64, _vp, _i64, _vp],
    "hpcla_axpby_f64": [_f64, _vp, _f64, _vp, _vp, _i64, _vp],
    "hpcla_merge_combine_f64_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_merge_combine_f64_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "hpcla_fill_uniform_f64": [_vp, _i64, _i64, _u64, _vp],
    # Float32 element type (csrc/f32.hip)
    "hpcla_spmv_csr_f32_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp],
    "hpcla_spmv_csr_f32_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _vp],
    "hpcla_spmv_split_f32_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp],
    "hpcla_spmv_split_f32_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp],
    "hpcla_spmm_csr_f32_i32": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i32, _i32, _vp],
    "hpcla_spmm_csr_f32_i64": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _i32, _i32, _vp],
    "hpcla_spmm_split_f32_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_spmm_split_f32_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_spmv_dist_f32_i32": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp],
    "hpcla_spmv_dist_f32_i64": [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp],
    "hpcla_halo_begin_f32": [_vp, _vp, _vp, _vp],
    "hpcla_halo_begin_strided_f32": [_vp, _vp, _i64, _i64, _vp, _vp],
    "hpcla_spmm_split_colmajor_f32_i32": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_spmm_split_colmajor_f32_i64": [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _vp, _i64, _vp],
    "hpcla_transpose_f32": [_vp, _i64, _i32, _vp, _i64, _i32, _i64, _i64, _vp],
    "hpcla_dot_f32": [_vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_nrm2sq_f32": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_asum_f32": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_amax_f32": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_sum_f32": [_vp, _vp, _i64, _vp, _vp, _vp],
    "hpcla_maxval_f32": [_vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "hpcla_axpby_f32": [_f32, _vp, _f32, _vp, _vp, _i64, _vp],
    "hpcla_scale_f32": [_f32, _vp, _vp, _i64, _vp],
    "hpcla_divide_f32": [_vp, _f32, _vp, _i64, _vp],
}
_RESTYPES = {
    "hpcla_last_error": ctypes.c_char_p,
    "hpcla_reduce_work_bytes": _i64,
    "hpcla_spmv_dot_work_bytes": _i64,
    "hpcla_colspace_work_bytes": _i64,
    "hpcla_submatrix_work_bytes": _i64,
    "hpcla_submatrix_scan_chunk": _i64,
    "hpcla_select_short_cap": _i64,
    "hpcla_select_tile": _i64,
    "hpcla_select_work_bytes": _i64,
    "hpcla_rcm_frontier_cap": _i64,
    "hpcla_rcm_candidate_cap": _i64,
    "hpcla_rcm_work_bytes": _i64,
    "hpcla_assemble_chunk": _i64,
    "hpcla_assemble_run": _i64,
    "hpcla_assemble_pass": _i64,
    "hpcla_assemble_work_bytes": _i64,
    "hpcla_assemble_values_work_bytes": _i64,
    "hpcla_poisson2d_nnz": _i64,
    "hpcla_poisson3d_nnz": _i64,
    "hpcla_spgemm_bin_cap": _i64,
    "hpcla_gemv_t_work_bytes": _i64,
    "hpcla_gram_work_bytes": _i64,
    "hpcla_spmm_t_struct_work_bytes": _i64,
    "hpcla_spmm_runs_desc_bytes": _i64,
    "hpcla_spmv_longrows_work_bytes": _i64,
    "hpcla_cols16_padded_len": _i64,
    "hpcla_pcg_work_bytes": _i64,
    "hpcla_fsai_work_bytes": _i64,
    "hpcla_ilu_work_bytes": _i64,
    "hpcla_amg_work_bytes": _i64,
    "hpcla_amg_round_blocks": _i64,
    "hpcla_bicgstab_work_bytes": _i64,
    "hpcla_lsqr_work_bytes": _i64,
    "hpcla_minres_work_bytes": _i64,
    "hpcla_gmres_work_bytes": _i64,
    "hpcla_gmres_small_offset": _i64,
    "hpcla_eigsh_small_offset": _i64,
    "hpcla_svds_small_offset": _i64,
    "hpcla_lobpcg_chunk_rows": _i64,
    "hpcla_lobpcg_work_bytes": _i64,
    "hpcla_lobpcg_gen_work_bytes": _i64,
    "hpcla_qr_work_bytes": _i64,
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load() -> ctypes.CDLL:
    """Load libhpcla_rocm.so.  Inside a PyTorch process torch must be imported first so that the
    HIP runtime (libamdhip64.so.7) and librccl.so.1 already mapped by torch are the ones the
    library binds to (one HIP runtime per process: torch tensors' device pointers and streams are
    then directly usable)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C linearalgebrampi.jl_amd/csrc` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback.")
    try:
        import torch  # noqa: F401  (maps torch's libamdhip64 / librccl first)
    except Exception:  # pragma: no cover - torch is plumbing, the library works without it
        pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, ctypes.c_int)
    _lib = lib
    apply_spmv_sweep_env()
    return lib


def apply_spmv_sweep_env() -> None:
    """``HPCLA_SPMV_SWEEP=forward`` keeps every SpMV launch of this process forwards (the OFF leg of A/B measurements of the
    alternating sweep direction, csrc/spmv.hip next_sweep); ``alternate`` or unset: the library's default.  Applied when the
    library is loaded, through hpcla_set_spmv_sweep: the library itself reads no environment variable for it."""
    want = os.environ.get("HPCLA_SPMV_SWEEP", "alternate").strip().lower()
    call("hpcla_set_spmv_sweep", 0 if want.startswith("f") else -1)


def last_error() -> str:
    s = load().hpcla_last_error()
    return s.decode("utf-8", "replace") if s else ""


def check(fn_name: str, status: int) -> None:
    if status != OK:
        raise HPCLAError(fn_name, status, last_error())


def call(fn_name: str, *args) -> None:
    """Call a status-returning entry point and raise HPCLAError on failure."""
    check(fn_name, getattr(load(), fn_name)(*args))
