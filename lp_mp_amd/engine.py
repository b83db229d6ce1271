"""ctypes binding of the C ABI in include/lpmp_engine.h (liblpmp_engine.so).

No CPU fallback: ``Engine`` raises if the HIP extension is missing or no GPU is present.
``Plan`` (host-only analysis: ordering, weights, level schedule) works without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from . import build as _build
from .model import FlatModel

_LIB = None
N_KCLASS = 28
KCLASS_NAMES = ["generic", "dense4", "dense8", "dense16", "dense32", "potts4", "potts8", "potts16", "potts32",
                "dense_v4", "dense_v8", "dense_v16", "dense_v32", "potts_v4", "potts_v8", "potts_v16", "potts_v32",
                "dense_big", "small", "pairwise4", "pairwise8", "pairwise16", "pairwise32",
                "shared4", "shared8", "shared16", "shared32", "diff"]
# kernel symbols as rocprofv3 prints them: dense classes run the packed kernel (KMAX 2 at L >= 16, 4 below; packets for up
# to 8 active messages per factor, indirect records above); the _v classes (any label count up to
# the padded width, rectangular tables) are the same kernels with run-time dims; the exact dense kernels come in a
# plain and a non-temporal-access form (last template argument), chosen by the size of the model: the names below
# are prefixes
KERNEL_NAMES = ["sweep_generic_kernel<64>", "sweep_dense_pk_kernel<4, 4, false", "sweep_dense_pk_kernel<8, 4, false",
                "sweep_dense_pk_kernel<16, 2, false", "sweep_dense_pk_kernel<32, 2, false",
                "sweep_potts_pk_kernel<4, false", "sweep_potts_pk_kernel<8, false", "sweep_potts_pk_kernel<16, false",
                "sweep_potts_pk_kernel<32, false",
                "sweep_dense_pk_kernel<4, 4, true, false>", "sweep_dense_pk_kernel<8, 4, true, false>",
                "sweep_dense_pk_kernel<16, 2, true, false>", "sweep_dense_pk_kernel<32, 2, true, false>",
                "sweep_potts_pk_kernel<4, true, false>", "sweep_potts_pk_kernel<8, true, false>",
                "sweep_potts_pk_kernel<16, true, false>", "sweep_potts_pk_kernel<32, true, false>", "sweep_dense_big_kernel", "sweep_generic_kernel<1>",
                "sweep_pairwise_pk_kernel<4>", "sweep_pairwise_pk_kernel<8>", "sweep_pairwise_pk_kernel<16>",
                "sweep_pairwise_pk_kernel<32>",
                "sweep_shared_pk_kernel<4", "sweep_shared_pk_kernel<8", "sweep_shared_pk_kernel<16", "sweep_shared_pk_kernel<32",
                "sweep_diff_kernel"]
MEM_HOST, MEM_DEVICE = 0, 1
# lpmp_set_table_precision (include/lpmp_engine.h): how the entries of DENSE pairwise tables are stored on the device
TABLES_F64, TABLES_F32, TABLES_F32_ROUND = 0, 1, 2
TABLE_PRECISIONS = {"f64": TABLES_F64, "f32": TABLES_F32, "f32_round": TABLES_F32_ROUND}
# classes whose kernels read dense tables have an f32 kernel of their own (name: ..._f32_kernel, same template arguments)
_F32_KERNEL_CLASSES = set(range(1, 5)) | set(range(9, 13)) | {17} | set(range(19, 23))


def _table_precision_code(p) -> int:
    if isinstance(p, str):
        if p not in TABLE_PRECISIONS:
            raise ValueError(f"table_precision: one of {sorted(TABLE_PRECISIONS)}, not {p!r}")
        return TABLE_PRECISIONS[p]
    return int(p)

EXPORTS = [
    "lpmp_last_error", "lpmp_version", "lpmp_experiment_build", "lpmp_set_rows_layout", "lpmp_rows_layout", "lpmp_lower_bound_recomputed", "lpmp_plan_create", "lpmp_plan_destroy", "lpmp_plan_n_factors",
    "lpmp_plan_n_updated", "lpmp_plan_get_order", "lpmp_plan_get_update_order", "lpmp_plan_omega_nnz",
    "lpmp_plan_mask_nnz", "lpmp_plan_get_omega", "lpmp_plan_get_mask", "lpmp_plan_get_msg_lists",
    "lpmp_plan_anisotropic_weights", "lpmp_plan_schedule_info", "lpmp_plan_custom_schedule_info", "lpmp_plan_schedule_classes", "lpmp_plan_get_update_levels", "lpmp_plan_pass_schedule_info", "lpmp_plan_pass_rotates", "lpmp_plan_chain_info", "lpmp_plan_mailbox_info", "lpmp_plan_level_loop_info", "lpmp_create", "lpmp_destroy", "lpmp_set_stream",
    "lpmp_upload_model", "lpmp_set_reparametrization", "lpmp_set_reparametrization_type", "lpmp_set_inner_iterations", "lpmp_plan_get_partitions", "lpmp_compute_pass", "lpmp_compute_forward_pass",
    "lpmp_compute_backward_pass", "lpmp_compute_pass_custom", "lpmp_schedule_create", "lpmp_schedule_create_fused", "lpmp_schedule_run",
    "lpmp_schedule_info", "lpmp_schedule_destroy", "lpmp_lower_bound", "lpmp_factor_lower_bounds",
    "lpmp_invalidate_lower_bounds", "lpmp_synchronize", "lpmp_dual_size", "lpmp_download_duals", "lpmp_upload_duals", "lpmp_device_duals",
    "lpmp_engine_plan", "lpmp_engine_plan_mut", "lpmp_enable_kernel_timing", "lpmp_get_kernel_timing",
    "lpmp_reset_kernel_timing", "lpmp_get_chain_launches", "lpmp_prepare_passes", "lpmp_synth_fill", "lpmp_compute_forward_pass_and_primal",
    "lpmp_compute_backward_pass_and_primal", "lpmp_compute_pass_and_primal", "lpmp_check_primal_consistency",
    "lpmp_evaluate_primal", "lpmp_download_primal", "lpmp_upload_primal", "lpmp_streaming_access",
    "lpmp_boundary_create", "lpmp_boundary_destroy", "lpmp_boundary_out_doubles", "lpmp_boundary_in_doubles", "lpmp_boundary_pack",
    "lpmp_boundary_reply", "lpmp_boundary_fold", "lpmp_engine_stream", "lpmp_synth_fill_blocks",
    "lpmp_halo_create", "lpmp_halo_destroy", "lpmp_halo_out_doubles", "lpmp_halo_in_doubles", "lpmp_halo_pack", "lpmp_halo_unpack",
    "lpmp_set_speculation", "lpmp_speculation_stats", "lpmp_chain_cache_bytes",
    "lpmp_set_persistent_launches", "lpmp_persistent_launches", "lpmp_device_identity",
    "lpmp_plan_suggest_order", "lpmp_graph_colour_major_order", "lpmp_graph_refine_partition",
    "lpmp_set_table_precision", "lpmp_table_precision", "lpmp_plan_set_table_precision",
    "lpmp_plan_n_shared_tables", "lpmp_plan_get_diff_band", "lpmp_plan_diff_band_info", "lpmp_get_diff_band_launches", "lpmp_get_diff_shift_launches",
    "lpmp_plan_get_diff_shift_band", "lpmp_plan_diff_shift_band_info", "lpmp_get_diff_shift_band_launches",
    "lpmp_upload_costs", "lpmp_set_vectors", "lpmp_zero_pairwise_duals", "lpmp_schedules_built",
    "lpmp_plan_set_shared_pool", "lpmp_upload_shared_pool", "lpmp_set_constants",
    "lpmp_plan_peer_minima", "lpmp_get_peer_minima_launches",
    "lpmp_decode_primal", "lpmp_plan_decode_info", "lpmp_plan_get_decode_levels",
    "lpmp_readout_create", "lpmp_readout_destroy", "lpmp_readout_n", "lpmp_readout_max_labels",
    "lpmp_readout_labels", "lpmp_readout_vectors", "lpmp_readout_beliefs",
    "lpmp_window_set_create", "lpmp_window_set_destroy", "lpmp_window_set_n", "lpmp_window_set_max_labels", "lpmp_window_set_n_pairwise",
    "lpmp_move_windows", "lpmp_plan_window_info",
    "lpmp_path_set_create", "lpmp_path_set_destroy", "lpmp_path_set_n_groups", "lpmp_path_set_n_paths", "lpmp_path_set_longest",
    "lpmp_path_set_scratch_bytes", "lpmp_path_moves", "lpmp_plan_path_info",
    "lpmp_forest_set_create", "lpmp_forest_set_destroy", "lpmp_forest_set_n_groups", "lpmp_forest_set_n_trees", "lpmp_forest_set_max_height",
    "lpmp_forest_set_scratch_bytes", "lpmp_forest_moves", "lpmp_plan_forest_info", "lpmp_plan_suggest_forests",
    "lpmp_readout_set_labels", "lpmp_move_windows_carry", "lpmp_lower_bound_dev", "lpmp_evaluate_primal_dev",
]


def library_path() -> str:
    # LPMP_ENGINE_SO: load another build of the library (an older revision, for an A/B); never a CPU path
    return os.environ.get("LPMP_ENGINE_SO", _build.SO)


def lib():
    """Loads the HIP extension; raises (never falls back) if it is not built."""
    global _LIB
    if _LIB is None:
        # torch ships its own HIP runtime; it must be the one the process loads first, otherwise torch
        # finds no GPU once another libamdhip64 has initialised the device
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        so = library_path()
        if not os.path.exists(so):
            raise RuntimeError(f"{so} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the engine has no CPU fallback)")
        L = C.CDLL(so)
        L.lpmp_last_error.restype = C.c_char_p
        L.lpmp_version.restype = C.c_char_p
        for n in ("lpmp_plan_n_factors", "lpmp_dual_size"):
            getattr(L, n).restype = C.c_int64
            getattr(L, n).argtypes = [C.c_void_p]
        for n in ("lpmp_plan_n_updated", "lpmp_plan_omega_nnz", "lpmp_plan_mask_nnz"):
            getattr(L, n).restype = C.c_int64
            getattr(L, n).argtypes = [C.c_void_p, C.c_int]
        L.lpmp_plan_create.argtypes = [C.c_void_p, C.c_void_p]
        L.lpmp_plan_destroy.argtypes = [C.c_void_p]
        L.lpmp_plan_get_order.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.lpmp_plan_get_update_order.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.lpmp_plan_get_omega.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.lpmp_plan_get_mask.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.lpmp_plan_get_msg_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.lpmp_plan_anisotropic_weights.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8
        L.lpmp_plan_schedule_info.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.lpmp_plan_pass_schedule_info.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.lpmp_plan_pass_rotates.argtypes = [C.c_void_p, C.c_int]
        L.lpmp_plan_chain_info.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
        L.lpmp_plan_mailbox_info.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 2
        L.lpmp_plan_level_loop_info.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.lpmp_plan_get_update_levels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.lpmp_plan_schedule_classes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.lpmp_plan_custom_schedule_info.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5
        L.lpmp_create.argtypes = [C.c_int, C.c_void_p]
        L.lpmp_destroy.argtypes = [C.c_void_p]
        L.lpmp_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.lpmp_upload_model.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.lpmp_set_reparametrization.argtypes = [C.c_void_p, C.c_int]
        L.lpmp_set_reparametrization_type.argtypes = [C.c_void_p, C.c_int]
        L.lpmp_set_inner_iterations.argtypes = [C.c_void_p, C.c_int]
        L.lpmp_plan_get_partitions.argtypes = [C.c_void_p] * 4
        L.lpmp_compute_pass.argtypes = [C.c_void_p, C.c_int]
        L.lpmp_compute_forward_pass.argtypes = [C.c_void_p]
        L.lpmp_compute_backward_pass.argtypes = [C.c_void_p]
        L.lpmp_compute_pass_custom.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        L.lpmp_schedule_create.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        L.lpmp_schedule_create_fused.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        L.lpmp_schedule_run.argtypes = [C.c_void_p, C.c_int]
        L.lpmp_schedule_info.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.lpmp_schedule_destroy.argtypes = [C.c_void_p, C.c_int]
        L.lpmp_lower_bound.argtypes = [C.c_void_p, C.c_void_p]
        L.lpmp_factor_lower_bounds.argtypes = [C.c_void_p, C.c_void_p]
        L.lpmp_invalidate_lower_bounds.argtypes = [C.c_void_p]
        L.lpmp_synchronize.argtypes = [C.c_void_p]
        L.lpmp_download_duals.argtypes = [C.c_void_p, C.c_void_p]
        L.lpmp_upload_duals.argtypes = [C.c_void_p, C.c_void_p]
        L.lpmp_device_duals.restype = C.c_void_p
        L.lpmp_device_duals.argtypes = [C.c_void_p]
        L.lpmp_engine_plan.restype = C.c_void_p
        L.lpmp_engine_plan.argtypes = [C.c_void_p]
        L.lpmp_engine_plan_mut.restype = C.c_void_p
        L.lpmp_engine_plan_mut.argtypes = [C.c_void_p]
        for name in ("lpmp_compute_forward_pass_and_primal", "lpmp_compute_backward_pass_and_primal", "lpmp_compute_pass_and_primal"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_uint64]
        for name in ("lpmp_check_primal_consistency", "lpmp_evaluate_primal", "lpmp_download_primal", "lpmp_upload_primal"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p]
        L.lpmp_streaming_access.argtypes = [C.c_void_p]
        L.lpmp_enable_kernel_timing.argtypes = [C.c_void_p, C.c_int]
        L.lpmp_get_kernel_timing.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.lpmp_reset_kernel_timing.argtypes = [C.c_void_p]
        L.lpmp_get_chain_launches.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.lpmp_prepare_passes.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "lpmp_set_speculation"):       # (absent only in an older experimental build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_set_speculation.argtypes = [C.c_void_p, C.c_int]
            L.lpmp_speculation_stats.argtypes = [C.c_void_p] + [C.c_void_p] * 4
            L.lpmp_chain_cache_bytes.restype = C.c_int64
            L.lpmp_chain_cache_bytes.argtypes = [C.c_void_p]
        if hasattr(L, "lpmp_lower_bound_recomputed"):
            L.lpmp_lower_bound_recomputed.restype = C.c_int64
            L.lpmp_lower_bound_recomputed.argtypes = [C.c_void_p]
        if hasattr(L, "lpmp_set_rows_layout"):
            L.lpmp_set_rows_layout.argtypes = [C.c_void_p, C.c_int]
            L.lpmp_rows_layout.argtypes = [C.c_void_p]
        if hasattr(L, "lpmp_set_table_precision"):   # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_set_table_precision.argtypes = [C.c_void_p, C.c_int]
            L.lpmp_table_precision.argtypes = [C.c_void_p]
            L.lpmp_plan_set_table_precision.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "lpmp_set_persistent_launches"):
            L.lpmp_set_persistent_launches.argtypes = [C.c_void_p, C.c_int]
            L.lpmp_persistent_launches.argtypes = [C.c_void_p]
            L.lpmp_device_identity.argtypes = [C.c_int, C.c_char_p, C.c_int64]
        if hasattr(L, "lpmp_plan_get_diff_band"):    # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_plan_n_shared_tables.argtypes = [C.c_void_p]
            L.lpmp_plan_get_diff_band.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
            L.lpmp_plan_diff_band_info.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
            L.lpmp_get_diff_band_launches.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "lpmp_get_diff_shift_launches"):   # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_get_diff_shift_launches.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "lpmp_plan_get_diff_shift_band"):   # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_plan_get_diff_shift_band.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
            L.lpmp_plan_diff_shift_band_info.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
            L.lpmp_get_diff_shift_band_launches.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "lpmp_plan_peer_minima"):      # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_plan_peer_minima.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
            L.lpmp_get_peer_minima_launches.argtypes = [C.c_void_p, C.c_void_p]
        if hasattr(L, "lpmp_upload_costs"):          # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_upload_costs.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            L.lpmp_set_vectors.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int]
            L.lpmp_zero_pairwise_duals.argtypes = [C.c_void_p]
            L.lpmp_schedules_built.restype = C.c_int64
            L.lpmp_schedules_built.argtypes = [C.c_void_p]
        if hasattr(L, "lpmp_set_constants"):         # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_plan_set_shared_pool.argtypes = [C.c_void_p, C.c_void_p]
            L.lpmp_upload_shared_pool.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            L.lpmp_set_constants.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        if hasattr(L, "lpmp_decode_primal"):         # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_decode_primal.argtypes = [C.c_void_p, C.c_int, C.c_int]
            L.lpmp_plan_decode_info.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
            L.lpmp_plan_get_decode_levels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(L, "lpmp_readout_create"):        # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_readout_create.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            L.lpmp_readout_destroy.restype = None
            L.lpmp_readout_destroy.argtypes = [C.c_void_p]
            L.lpmp_readout_n.restype = C.c_int64
            L.lpmp_readout_n.argtypes = [C.c_void_p]
            L.lpmp_readout_max_labels.restype = C.c_int32
            L.lpmp_readout_max_labels.argtypes = [C.c_void_p]
            L.lpmp_readout_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
            L.lpmp_readout_vectors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
            L.lpmp_readout_beliefs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
        if hasattr(L, "lpmp_move_windows"):          # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_window_set_create.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            L.lpmp_window_set_destroy.restype = None
            L.lpmp_window_set_destroy.argtypes = [C.c_void_p]
            for n in ("lpmp_window_set_n", "lpmp_window_set_n_pairwise"):
                getattr(L, n).restype = C.c_int64
                getattr(L, n).argtypes = [C.c_void_p]
            L.lpmp_window_set_max_labels.restype = C.c_int32
            L.lpmp_window_set_max_labels.argtypes = [C.c_void_p]
            L.lpmp_move_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
            L.lpmp_plan_window_info.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
        if hasattr(L, "lpmp_path_set_create"):       # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_path_set_create.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4
            L.lpmp_path_set_destroy.restype = None
            L.lpmp_path_set_destroy.argtypes = [C.c_void_p]
            for n in ("lpmp_path_set_n_groups", "lpmp_path_set_n_paths", "lpmp_path_set_longest", "lpmp_path_set_scratch_bytes"):
                getattr(L, n).restype = C.c_int64
                getattr(L, n).argtypes = [C.c_void_p]
            L.lpmp_path_moves.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            L.lpmp_plan_path_info.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + [C.c_char_p, C.c_int]
        if hasattr(L, "lpmp_forest_set_create"):     # (absent only in an older build loaded through LPMP_ENGINE_SO for an A/B)
            L.lpmp_forest_set_create.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4
            L.lpmp_forest_set_destroy.restype = None
            L.lpmp_forest_set_destroy.argtypes = [C.c_void_p]
            for n in ("lpmp_forest_set_n_groups", "lpmp_forest_set_n_trees", "lpmp_forest_set_max_height", "lpmp_forest_set_scratch_bytes"):
                getattr(L, n).restype = C.c_int64
                getattr(L, n).argtypes = [C.c_void_p]
            L.lpmp_forest_moves.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            L.lpmp_plan_forest_info.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7 + [C.c_char_p, C.c_int]
            L.lpmp_plan_suggest_forests.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        if hasattr(L, "lpmp_readout_set_labels"):    # primal state on the device (absent only in an older build loaded for an A/B)
            L.lpmp_readout_set_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
            L.lpmp_move_windows_carry.argtypes = L.lpmp_move_windows.argtypes
            L.lpmp_lower_bound_dev.argtypes = [C.c_void_p, C.c_void_p]
            L.lpmp_evaluate_primal_dev.argtypes = [C.c_void_p, C.c_void_p]
        L.lpmp_plan_suggest_order.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.lpmp_graph_colour_major_order.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.lpmp_graph_refine_partition.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_uint64, C.c_void_p]
        L.lpmp_synth_fill.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p]
        L.lpmp_synth_fill_blocks.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p]
        L.lpmp_boundary_create.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5
        L.lpmp_boundary_destroy.argtypes = [C.c_void_p]
        for n in ("lpmp_boundary_out_doubles", "lpmp_boundary_in_doubles"):
            getattr(L, n).restype = C.c_int64
            getattr(L, n).argtypes = [C.c_void_p]
        L.lpmp_boundary_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.lpmp_boundary_reply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lpmp_boundary_fold.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.lpmp_engine_stream.restype = C.c_void_p
        L.lpmp_engine_stream.argtypes = [C.c_void_p]
        L.lpmp_halo_create.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lpmp_halo_destroy.argtypes = [C.c_void_p]
        for n in ("lpmp_halo_out_doubles", "lpmp_halo_in_doubles"):
            getattr(L, n).restype = C.c_int64
            getattr(L, n).argtypes = [C.c_void_p]
        L.lpmp_halo_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.lpmp_halo_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


class EngineError(RuntimeError):
    """Mirrors the std::runtime_error the reference throws (LP_MP.h:458)."""

    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


def _chk(rc: int):
    if rc != 0:
        raise EngineError(rc, lib().lpmp_last_error().decode())


class Plan:
    """Host-only analysis of a model: orderings, weights, level schedule (no GPU needed)."""

    def __init__(self, model: Optional[FlatModel] = None, _handle=None, _owner=None, table_precision=None):
        """``table_precision``: "f64" (default) / "f32" / "f32_round" — the byte accounting of a device that stores the dense
        tables as floats (lpmp_plan_set_table_precision); classes, levels and records do not depend on it"""
        self.L = lib()
        self._owner = _owner
        if _handle is not None:
            self.h = _handle
            self._own = False
        else:
            cs = model.c_struct()
            h = C.c_void_p()
            _chk(self.L.lpmp_plan_create(C.addressof(cs), C.addressof(h)))
            self.h = h.value
            self._own = True
            if table_precision is not None:
                _chk(self.L.lpmp_plan_set_table_precision(self.h, _table_precision_code(table_precision)))

    def __del__(self):
        if getattr(self, "_own", False) and getattr(self, "h", None):
            self.L.lpmp_plan_destroy(self.h)
            self.h = None

    @property
    def n_factors(self) -> int:
        return self.L.lpmp_plan_n_factors(self.h)

    def order(self, d: int) -> np.ndarray:
        out = np.empty(self.n_factors, np.int32)
        _chk(self.L.lpmp_plan_get_order(self.h, d, out.ctypes.data))
        return out

    def update_order(self, d: int) -> np.ndarray:
        out = np.empty(self.L.lpmp_plan_n_updated(self.h, d), np.int32)
        _chk(self.L.lpmp_plan_get_update_order(self.h, d, out.ctypes.data))
        return out

    def omega(self, d: int, mode: int):
        off = np.empty(self.L.lpmp_plan_n_updated(self.h, d) + 1, np.int64)
        data = np.empty(self.L.lpmp_plan_omega_nnz(self.h, d), np.float64)
        _chk(self.L.lpmp_plan_get_omega(self.h, d, mode, off.ctypes.data, data.ctypes.data))
        return off, data

    def mask(self, d: int, mode: int):
        off = np.empty(self.L.lpmp_plan_n_updated(self.h, d) + 1, np.int64)
        data = np.empty(self.L.lpmp_plan_mask_nnz(self.h, d), np.uint8)
        _chk(self.L.lpmp_plan_get_mask(self.h, d, mode, off.ctypes.data, data.ctypes.data))
        return off, data

    def msg_lists(self, n_messages: int):
        off = np.empty(self.n_factors + 1, np.int64)
        ent = np.empty(2 * n_messages, np.int64)
        _chk(self.L.lpmp_plan_get_msg_lists(self.h, off.ctypes.data, ent.ctypes.data))
        return off, ent

    def anisotropic_weights(self, factors):
        factors = np.ascontiguousarray(factors, np.int32)
        nr, a, b = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(self.L.lpmp_plan_anisotropic_weights(self.h, factors.shape[0], factors.ctypes.data, C.addressof(nr),
                                                  C.addressof(a), C.addressof(b), None, None, None, None))
        om_off, mk_off = np.empty(nr.value + 1, np.int64), np.empty(nr.value + 1, np.int64)
        om, mk = np.empty(a.value, np.float64), np.empty(b.value, np.uint8)
        _chk(self.L.lpmp_plan_anisotropic_weights(self.h, factors.shape[0], factors.ctypes.data, None, None, None,
                                                  om_off.ctypes.data, om.ctypes.data, mk_off.ctypes.data, mk.ctypes.data))
        return om_off, om, mk_off, mk

    def update_levels(self, d: int, mode: int) -> np.ndarray:
        out = np.empty(self.L.lpmp_plan_n_updated(self.h, d), np.int32)
        _chk(self.L.lpmp_plan_get_update_levels(self.h, d, mode, out.ctypes.data))
        return out

    def schedule_info(self, d: int, mode: int) -> dict:
        v = [C.c_int64() for _ in range(5)]
        _chk(self.L.lpmp_plan_schedule_info(self.h, d, mode, *[C.addressof(x) for x in v]))
        return dict(zip(("n_levels", "n_launches", "n_receives", "n_sends", "algorithmic_bytes"), [x.value for x in v]))


def _custom_schedule_info(self, factors, om_off, om, mk_off, mk, fuse: bool = False) -> dict:
    """summary of the schedule an iterator-range pass (factor list, weight rows, receive-mask rows) compiles to"""
    factors = np.ascontiguousarray(factors, np.int32)
    om_off = np.ascontiguousarray(om_off, np.int64); om = np.ascontiguousarray(om, np.float64)
    mk_off = np.ascontiguousarray(mk_off, np.int64); mk = np.ascontiguousarray(mk, np.uint8)
    v = [C.c_int64() for _ in range(5)]
    _chk(self.L.lpmp_plan_custom_schedule_info(self.h, factors.shape[0], factors.ctypes.data, om_off.ctypes.data, om.ctypes.data,
                                               mk_off.ctypes.data, mk.ctypes.data, int(bool(fuse)), *[C.addressof(x) for x in v]))
    return dict(zip(("n_levels", "n_launches", "n_receives", "n_sends", "algorithmic_bytes"), [x.value for x in v]))


Plan.custom_schedule_info = _custom_schedule_info


def _schedule_classes(self, d: int, mode: int) -> dict:
    """updated factors of the sweep per device kernel class (only the classes that occur)"""
    out = np.zeros(N_KCLASS, np.int64)
    _chk(self.L.lpmp_plan_schedule_classes(self.h, d, mode, out.ctypes.data))
    return {KCLASS_NAMES[c]: int(out[c]) for c in range(N_KCLASS) if out[c]}


Plan.schedule_classes = _schedule_classes


def _diff_bands(self) -> dict:
    """{pool entry: (lo, hi, banded)} for every entry a DIFF factor references: the band of the vector as ``model.diff_band``
    states it, and whether its width is within the rule of the banded kernel"""
    out = {}
    for t in range(self.L.lpmp_plan_n_shared_tables(self.h)):
        lo, hi, banded = C.c_int32(), C.c_int32(), C.c_int()
        _chk(self.L.lpmp_plan_get_diff_band(self.h, t, C.addressof(lo), C.addressof(hi), C.addressof(banded)))
        if banded.value >= 0:
            out[t] = (lo.value, hi.value, bool(banded.value))
    return out


def _diff_band_info(self, d: int, mode: int) -> dict:
    """launches / receives of class diff in the sweep, and how many of them run the banded kernel"""
    v = [C.c_int64() for _ in range(4)]
    _chk(self.L.lpmp_plan_diff_band_info(self.h, d, mode, *[C.addressof(x) for x in v]))
    return dict(zip(("diff_launches", "band_launches", "diff_receives", "band_receives"), [x.value for x in v]))


def _diff_shift_bands(self) -> dict:
    """{pool entry: (lo, hi)} for every entry a DIFF_SHIFT factor references: the band of the vector itself, as ``model.diff_band``
    states it.  Whether a receive is banded depends on its dims too (``model.diff_shift_is_banded``), never on its shift"""
    out = {}
    for t in range(self.L.lpmp_plan_n_shared_tables(self.h)):
        lo, hi, ref = C.c_int32(), C.c_int32(), C.c_int()
        _chk(self.L.lpmp_plan_get_diff_shift_band(self.h, t, C.addressof(lo), C.addressof(hi), C.addressof(ref)))
        if ref.value:
            out[t] = (lo.value, hi.value)
    return out


def _diff_shift_band_info(self, d: int, mode: int) -> dict:
    """launches / receives of class diff with a DIFF_SHIFT factor in the sweep, and how many of them run the shifted banded kernel"""
    v = [C.c_int64() for _ in range(4)]
    _chk(self.L.lpmp_plan_diff_shift_band_info(self.h, d, mode, *[C.addressof(x) for x in v]))
    return dict(zip(("shift_launches", "shift_band_launches", "shift_receives", "shift_band_receives"), [x.value for x in v]))


def _set_shared_pool(self, sh_data):
    """new VALUES for the pool of this plan (lpmp_plan_set_shared_pool): ``sh_data`` packed as ``FlatModel.sh_data``.  The bands of
    the DIFF vectors and the kernel choice of every cached launch of class diff follow; nothing else of a schedule moves.  None is
    passed through as a null pointer (refused).  For a stand-alone plan: the plan of an engine (``Engine.plan``) is swapped together
    with the device copy of the pool by ``Engine.upload_shared_pool``."""
    if sh_data is None:
        _chk(self.L.lpmp_plan_set_shared_pool(self.h, None))
        return
    sh = np.ascontiguousarray(sh_data, np.float64).reshape(-1)
    _chk(self.L.lpmp_plan_set_shared_pool(self.h, C.c_void_p(sh.ctypes.data)))


Plan.set_shared_pool = _set_shared_pool
Plan.diff_bands = _diff_bands
Plan.diff_band_info = _diff_band_info
Plan.diff_shift_bands = _diff_shift_bands
Plan.diff_shift_band_info = _diff_shift_band_info


def _pass_info(self, mode: int) -> dict:
    v = [C.c_int64() for _ in range(5)]
    _chk(self.L.lpmp_plan_pass_schedule_info(self.h, mode, *[C.addressof(x) for x in v]))
    return dict(zip(("n_levels", "n_launches", "n_receives", "n_sends", "algorithmic_bytes"), [x.value for x in v]))


Plan.pass_schedule_info = _pass_info


def _peer_minima(self, mode: int):
    """(eligible, why): does the STRUCTURE of this mode's joined passes allow the peer-minima form (lpmp_plan_peer_minima)?
    why: "" or the first obstacle.  The engine further needs f64 tables in the packed layout."""
    buf = C.create_string_buffer(256)
    r = self.L.lpmp_plan_peer_minima(self.h, mode, buf, 256)
    if r < 0:
        _chk(r)
    return bool(r), buf.value.decode()


Plan.peer_minima = _peer_minima


def _pass_rotates(self, mode: int) -> bool:
    """does lpmp_compute_pass(n >= 2) join consecutive passes at their seam for this mode?"""
    r = self.L.lpmp_plan_pass_rotates(self.h, mode)
    if r < 0:
        _chk(r)
    return bool(r)


Plan.pass_rotates = _pass_rotates


def _chain_info(self, d: int, mode: int) -> dict:
    """how the chain executor runs a deep sweep (d = 0 / 1, or -1: the fused pass): persistent launches, tickets,
    dependencies, launches that stay plain (all 0: ordinary launches / graph replay)"""
    v = [C.c_int64() for _ in range(4)]
    _chk(self.L.lpmp_plan_chain_info(self.h, d, mode, *[C.addressof(x) for x in v]))
    w = [C.c_int64() for _ in range(2)]
    _chk(self.L.lpmp_plan_mailbox_info(self.h, d, mode, *[C.addressof(x) for x in w]))
    return dict(zip(("n_chains", "n_tickets", "n_dependencies", "n_plain_launches", "mailbox_rows", "mailbox_receives"), [x.value for x in v + w]))


Plan.chain_info = _chain_info


def _level_loop_info(self, d: int, mode: int) -> dict:
    """which body the launches of a sweep's level loops take (lpmp_plan_level_loop_info; d = 0 / 1, or -1: the fused pass):
    ``launches`` of all level loops, ``lane_launches`` of the lane-per-factor class, of these ``label_ops`` with one lane per op,
    of these ``label_paired`` (every message received, then sent) and ``label_staged`` (at most 16 records: staged in LDS under
    the shared send rule), ``label_paired_staged`` both.  ``lane_launches - label_ops`` launches run one lane per factor."""
    v = [C.c_int64() for _ in range(6)]
    _chk(self.L.lpmp_plan_level_loop_info(self.h, d, mode, *[C.addressof(x) for x in v]))
    return dict(zip(("launches", "lane_launches", "label_ops", "label_paired", "label_staged", "label_paired_staged"), [x.value for x in v]))


Plan.level_loop_info = _level_loop_info


def _partitions(self):
    """LP::construct_factor_partition (reference LP_MP.h:1717-1822): the components of the put_in_same_partition
    graph as arrays of (updated) factor indices"""
    n = C.c_int64()
    _chk(self.L.lpmp_plan_get_partitions(self.h, C.addressof(n), None, None))
    off = np.empty(n.value + 1, np.int64)
    f = np.empty(max(1, self.L.lpmp_plan_n_updated(self.h, 0)), np.int32)
    _chk(self.L.lpmp_plan_get_partitions(self.h, C.addressof(n), off.ctypes.data, f.ctypes.data))
    return [f[off[i]:off[i + 1]].copy() for i in range(n.value)]


Plan.partitions = _partitions


def _suggest_order(self, seed: int = 0):
    """(rank_of_factor[n_factors], number of colours): an order of all factors with the updated ones colour by colour
    (include/lpmp_engine.h, lpmp_plan_suggest_order); model.with_factor_order(rank) applies it"""
    rank = np.empty(self.n_factors, np.int32)
    k = C.c_int32()
    _chk(self.L.lpmp_plan_suggest_order(self.h, C.c_uint64(seed), rank.ctypes.data, C.addressof(k)))
    return rank, k.value


Plan.suggest_order = _suggest_order


def _decode_info(self, d: int) -> dict:
    """structure of ``Engine.decode_primal`` in direction d (lpmp_plan_decode_info): decoded unaries, dependent levels (one launch
    step each), unary-pairwise links.  EngineError (LPMP_ERR_UNSUPPORTED, naming the factor) for a model the decode refuses."""
    v = [C.c_int64() for _ in range(3)]
    _chk(self.L.lpmp_plan_decode_info(self.h, d, *[C.addressof(x) for x in v]))
    return dict(zip(("n_unaries", "n_levels", "n_links"), [x.value for x in v]))


def _decode_levels(self, d: int):
    """(factors, levels): the decoded unaries in decode order and the 1-based level of each (lpmp_plan_get_decode_levels)"""
    n = self.decode_info(d)["n_unaries"]
    f, lv = np.empty(n, np.int32), np.empty(n, np.int32)
    _chk(self.L.lpmp_plan_get_decode_levels(self.h, d, f.ctypes.data, lv.ctypes.data))
    return f, lv


Plan.decode_info = _decode_info
Plan.decode_levels = _decode_levels


def _window_info(self, factors=None) -> dict:
    """structure of ``Engine.window_set(factors)`` (lpmp_plan_window_info; None: every VECTOR factor): ``n_links`` unary-pairwise
    links of the listed factors, ``n_pairwise`` DIFF_SHIFT factors whose shift a move may write.  EngineError: LPMP_ERR_INVALID
    naming the entry (out of range, not a VECTOR factor, listed twice), LPMP_ERR_UNSUPPORTED naming the lowest listed factor the
    move does not take."""
    v = [C.c_int64() for _ in range(2)]
    buf = C.create_string_buffer(512)
    if factors is None:
        n, ptr = 0, None
    else:
        factors = np.ascontiguousarray(factors, np.int32).reshape(-1)
        keep = factors if factors.shape[0] else np.zeros(1, np.int32)
        n, ptr = int(factors.shape[0]), keep.ctypes.data
    _chk(self.L.lpmp_plan_window_info(self.h, n, ptr, C.addressof(v[0]), C.addressof(v[1]), buf, 512))
    return dict(n_links=v[0].value, n_pairwise=v[1].value)


Plan.window_info = _window_info


def flatten_path_groups(groups):
    """(group_off [n_groups + 1] int64 in paths, path_off [n_paths + 1] int64 in entries, unaries int32) of ``groups``: a sequence of
    groups, each a sequence of paths, each a sequence of factor indices — the arrays of lpmp_path_set_create"""
    group_off, path_off, un = [0], [0], []
    for g in groups:
        for path in g:
            un.extend(int(f) for f in path)
            path_off.append(len(un))
        group_off.append(len(path_off) - 1)
    if un and (min(un) < -(1 << 31) or max(un) >= (1 << 31)):
        raise ValueError("path groups: a factor index does not fit an int32")
    return np.asarray(group_off, np.int64), np.asarray(path_off, np.int64), np.asarray(un if un else [0], np.int32)[:len(un)]


def _path_info(self, groups) -> dict:
    """structure of ``Engine.path_set(groups)`` (lpmp_plan_path_info): ``n_paths``, ``n_path_edges`` (pairwise factors the recursion
    reads as tables) and ``n_off_path_links`` (cost lines a move reads).  EngineError with the refusals of lpmp_path_set_create:
    LPMP_ERR_INVALID naming the entry, LPMP_ERR_UNSUPPORTED naming the lowest listed factor a move does not take."""
    go, po, un = flatten_path_groups(groups)
    keep = un if un.shape[0] else np.zeros(1, np.int32)      # (an empty list: still a valid pointer)
    v = [C.c_int64() for _ in range(3)]
    buf = C.create_string_buffer(512)
    _chk(self.L.lpmp_plan_path_info(self.h, int(go.shape[0]) - 1, go.ctypes.data, po.ctypes.data, keep.ctypes.data,
                                    *[C.addressof(x) for x in v], buf, 512))
    return dict(zip(("n_paths", "n_path_edges", "n_off_path_links"), [x.value for x in v]))


Plan.path_info = _path_info


def flatten_forest_groups(groups):
    """(group_off [n_groups + 1] int64 in entries, unaries int32, parent int32) of ``groups``: a sequence of (unaries, parent) pairs
    of equally long sequences — parent[i] the factor index of the parent of unaries[i], -1 for a root — the arrays of
    lpmp_forest_set_create"""
    group_off, un, par = [0], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for u, q in groups:
        u, q = np.asarray(u, np.int64).reshape(-1), np.asarray(q, np.int64).reshape(-1)
        if u.shape[0] != q.shape[0]:
            raise ValueError("forest groups: %d unaries with %d parents" % (u.shape[0], q.shape[0]))
        un.append(u); par.append(q)
        group_off.append(group_off[-1] + u.shape[0])
    un, par = np.concatenate(un), np.concatenate(par)
    for x in (un, par):
        if x.shape[0] and (x.min() < -(1 << 31) or x.max() >= (1 << 31)):
            raise ValueError("forest groups: a factor index does not fit an int32")
    return np.asarray(group_off, np.int64), un.astype(np.int32), par.astype(np.int32)


def _valid_ptr(a):
    return a if a.shape[0] else np.zeros(1, a.dtype)      # (an empty list: still a valid pointer)


def _forest_info(self, groups) -> dict:
    """structure of ``Engine.forest_set(groups)`` (lpmp_plan_forest_info): ``n_trees``, ``n_tree_edges`` (pairwise factors the up
    sweep reads as tables), ``n_off_tree_links`` (cost lines a move reads) and ``max_height``.  EngineError with the refusals of
    lpmp_forest_set_create: LPMP_ERR_INVALID naming the entry, LPMP_ERR_UNSUPPORTED naming the lowest listed factor a move does
    not take."""
    go, un, par = flatten_forest_groups(groups)
    un, par = _valid_ptr(un), _valid_ptr(par)
    v = [C.c_int64() for _ in range(4)]
    buf = C.create_string_buffer(512)
    _chk(self.L.lpmp_plan_forest_info(self.h, int(go.shape[0]) - 1, go.ctypes.data, un.ctypes.data, par.ctypes.data,
                                      *[C.addressof(x) for x in v], buf, 512))
    return dict(zip(("n_trees", "n_tree_edges", "n_off_tree_links", "max_height"), [x.value for x in v]))


def _suggest_forests(self, max_groups: int = 0, left_out=None):
    """a cover of the model by forest groups for ``Engine.forest_set`` / ``LP.forest_moves`` (lpmp_plan_suggest_forests): a list
    of (unaries, parent) int32 array pairs, every tree rooted at a centre; deterministic.  ``max_groups`` > 0 stops after that
    many groups.  ``left_out`` (a list) receives the number of VECTOR factors a forest move does not take."""
    ng, ne, lo = C.c_int64(), C.c_int64(), C.c_int64()
    _chk(self.L.lpmp_plan_suggest_forests(self.h, int(max_groups), C.addressof(ng), C.addressof(ne), None, None, None, C.addressof(lo)))
    go = np.zeros(ng.value + 1, np.int64)
    un, par = np.zeros(max(ne.value, 1), np.int32), np.zeros(max(ne.value, 1), np.int32)
    _chk(self.L.lpmp_plan_suggest_forests(self.h, int(max_groups), None, None, go.ctypes.data, un.ctypes.data, par.ctypes.data, None))
    if left_out is not None:
        left_out.append(int(lo.value))
    return [(un[go[g]:go[g + 1]].copy(), par[go[g]:go[g + 1]].copy()) for g in range(ng.value)]


Plan.forest_info = _forest_info
Plan.suggest_forests = _suggest_forests


def graph_colour_major_order(n: int, edge_i, edge_j, seed: int = 0):
    """(rank[n] int64, number of colours): colour-major variable order of a pairwise graph on the planner's threads
    (lpmp_graph_colour_major_order; the numpy statement of the same algorithm is ordering.colour_major_order_numpy)"""
    ei = np.ascontiguousarray(edge_i, np.int64); ej = np.ascontiguousarray(edge_j, np.int64)
    assert ei.shape == ej.shape
    rank = np.empty(int(n), np.int64)
    k = C.c_int32()
    _chk(lib().lpmp_graph_colour_major_order(int(n), ei.shape[0], ei.ctypes.data, ej.ctypes.data, C.c_uint64(seed), rank.ctypes.data, C.addressof(k)))
    return rank, k.value


def graph_refine_partition(n: int, edge_i, edge_j, part, world: int, rounds: int = 30, imbalance: float = 0.03, seed: int = 0) -> np.ndarray:
    """balanced KL refinement of a k-way partition (lpmp_graph_refine_partition; numpy statement: multi_gpu.refine_partition)"""
    ei = np.ascontiguousarray(edge_i, np.int64); ej = np.ascontiguousarray(edge_j, np.int64)
    out = np.array(part, np.int64, copy=True)
    assert out.shape[0] == int(n)
    _chk(lib().lpmp_graph_refine_partition(int(n), ei.shape[0], ei.ctypes.data, ej.ctypes.data, int(world), int(rounds), float(imbalance), C.c_uint64(seed), out.ctypes.data))
    return out


class Engine:
    """Device engine. ``const_dev`` / ``dual_dev``: optional device pointers (ints) of caller-owned HBM
    buffers holding the packed pairwise tables / duals (zero-copy; the caller keeps them alive)."""

    def __init__(self, device: int = 0):
        self.L = lib()
        h = C.c_void_p()
        _chk(self.L.lpmp_create(int(device), C.addressof(h)))
        self.h = h.value
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.L.lpmp_destroy(self.h)
            self.h = None
            self._keep = None          # the caller-owned device buffers the engine borrowed may go now

    def __del__(self):
        self.close()

    def set_stream(self, stream_ptr: int):
        _chk(self.L.lpmp_set_stream(self.h, C.c_void_p(stream_ptr)))

    def upload(self, model: FlatModel, const_dev: Optional[int] = None, dual_dev: Optional[int] = None, keep=None, rows_layout: Optional[bool] = None,
               table_precision=None):
        """``rows_layout``: dense pairwise factors as [table | m1 | m2] rows of an engine-private buffer (lpmp_set_rows_layout);
        None: whatever LPMP_ROWS_LAYOUT says (default off).
        ``table_precision``: "f64" / "f32" (strict: every dense table entry must be exactly a float) / "f32_round" — dense tables as
        floats on the device, widened in the load, all arithmetic in double (lpmp_set_table_precision); None: as set before (f64)"""
        if rows_layout is not None:
            _chk(self.L.lpmp_set_rows_layout(self.h, 1 if rows_layout else 0))
        if table_precision is not None:
            _chk(self.L.lpmp_set_table_precision(self.h, _table_precision_code(table_precision)))
        cs = model.c_struct()
        if const_dev is not None:
            cs.const_data = const_dev
        if dual_dev is not None:
            cs.dual_data = dual_dev
        self._keep = keep
        self.model = model
        _chk(self.L.lpmp_upload_model(self.h, C.addressof(cs), MEM_DEVICE if const_dev is not None else MEM_HOST,
                                      MEM_DEVICE if dual_dev is not None else MEM_HOST))

    # ---- new costs on the plan that is already there (include/lpmp_engine.h): nothing is planned, every schedule stays ----
    def upload_costs(self, const=None, duals=None, const_dev: Optional[int] = None, dual_dev: Optional[int] = None):
        """Same structure, other numbers (lpmp_upload_costs).  ``const`` / ``duals``: numpy arrays packed as ``FlatModel.const_data`` /
        ``dual_data``; ``const_dev`` / ``dual_dev``: raw device pointers instead, as in ``upload`` (a pointer that is the buffer the
        engine already borrows is not copied: "rewritten in place").  A half that is not given stays as it is: constants alone are
        a warm start (the messages are kept).  ``self.model`` becomes a copy with the host arrays given; halves that came as device
        pointers keep the arrays of the upload there (the structure is what ``self.model`` is read for)."""
        import dataclasses
        n_const, n_dual = int(self.model.const_sizes().sum()), int(self.L.lpmp_dual_size(self.h))
        cp, cm, dp, dm = None, MEM_HOST, None, MEM_HOST
        if const_dev is not None:
            cp, cm = C.c_void_p(const_dev), MEM_DEVICE
        elif const is not None:
            const = np.ascontiguousarray(const, np.float64)
            if const.shape != (n_const,):
                raise ValueError(f"upload_costs: {n_const} constants expected, got an array of shape {const.shape}")
            if n_const == 0:
                const = np.zeros(1)                  # (a model without constants: a valid pointer that is never read, alive across the call)
            cp = C.c_void_p(const.ctypes.data)
        if dual_dev is not None:
            dp, dm = C.c_void_p(dual_dev), MEM_DEVICE
        elif duals is not None:
            duals = np.ascontiguousarray(duals, np.float64)
            if duals.shape != (n_dual,):
                raise ValueError(f"upload_costs: {n_dual} duals expected, got an array of shape {duals.shape}")
            dp = C.c_void_p(duals.ctypes.data)
        _chk(self.L.lpmp_upload_costs(self.h, cp, cm, dp, dm))
        new = {}
        if const_dev is None and const is not None and n_const:
            new["const_data"] = const
        if dual_dev is None and duals is not None:
            new["dual_data"] = duals
        if new:
            self.model = dataclasses.replace(self.model, _keep=[], **new)

    def set_vectors(self, factors, src=None, accumulate: bool = False, src_dev: Optional[int] = None, src_stride: Optional[int] = None):
        """theta of the listed VECTOR factors := (``accumulate``: +=) row i of ``src`` (lpmp_set_vectors).  ``src``: a 2-D numpy array
        [n, >= longest vector], or a 1-D one with ``src_stride``; ``src_dev``: a raw device pointer with ``src_stride`` instead."""
        factors = np.ascontiguousarray(factors, np.int32).reshape(-1)
        n = int(factors.shape[0])
        if src_dev is not None:
            if src_stride is None:
                raise ValueError("set_vectors: src_dev needs src_stride")
            ptr, mem = C.c_void_p(src_dev), MEM_DEVICE
        else:
            src = np.ascontiguousarray(src, np.float64)
            if src.ndim == 2:
                if src.shape[0] < n:
                    raise ValueError("set_vectors: fewer rows than factors")
                src_stride = src.shape[1] if src_stride is None else src_stride
            elif src_stride is None:
                raise ValueError("set_vectors: a flat source needs src_stride")
            if n > 0 and src.size < (n - 1) * int(src_stride) + 1:
                raise ValueError("set_vectors: source shorter than the rows it is said to hold")
            ptr, mem = C.c_void_p(src.ctypes.data), MEM_HOST
        _chk(self.L.lpmp_set_vectors(self.h, n, factors.ctypes.data, ptr, int(src_stride), mem, 1 if accumulate else 0))

    def upload_shared_pool(self, sh_data=None, sh_dev: Optional[int] = None):
        """New VALUES for the shared pool of the planned model (lpmp_upload_shared_pool): ``sh_data`` packed as ``FlatModel.sh_data``
        (same entries and dims), or ``sh_dev``: a raw device pointer to such an array.  Plans nothing; the duals stay.  With a host
        array ``self.model`` becomes ``self.model.with_pool(sh_data)``."""
        if sh_dev is not None:
            _chk(self.L.lpmp_upload_shared_pool(self.h, C.c_void_p(sh_dev), MEM_DEVICE))
            return
        if sh_data is None:
            _chk(self.L.lpmp_upload_shared_pool(self.h, None, MEM_HOST))
            return
        sh = np.ascontiguousarray(sh_data, np.float64).reshape(-1)
        have = getattr(getattr(self, "model", None), "sh_data", None)
        if have is not None and sh.shape != np.shape(have):
            raise ValueError(f"upload_shared_pool: a pool of {np.shape(have)[0]} entries expected, got {sh.shape[0]}")
        _chk(self.L.lpmp_upload_shared_pool(self.h, C.c_void_p(sh.ctypes.data), MEM_HOST))
        if have is not None:
            import dataclasses
            self.model = dataclasses.replace(self.model, sh_data=np.array(sh, copy=True), _keep=[])

    def set_constants(self, factors, src=None, src_dev: Optional[int] = None, src_stride: Optional[int] = None):
        """constants of the listed PAIRWISE factors := row i of ``src`` (lpmp_set_constants): a dense table row-major, or the one
        scalar of a Potts / SHARED / DIFF factor, or the two of a DIFF_SHIFT factor {scale, shift}.  ``src``: a 2-D numpy array [n, >= longest row], or a 1-D one with ``src_stride``;
        ``src_dev``: a raw device pointer with ``src_stride`` instead."""
        factors = np.ascontiguousarray(factors, np.int32).reshape(-1)
        n = int(factors.shape[0])
        if src_dev is not None:
            if src_stride is None:
                raise ValueError("set_constants: src_dev needs src_stride")
            ptr, mem = C.c_void_p(src_dev), MEM_DEVICE
        else:
            src = np.ascontiguousarray(src, np.float64)
            if src.ndim == 2:
                if src.shape[0] < n:
                    raise ValueError("set_constants: fewer rows than factors")
                src_stride = src.shape[1] if src_stride is None else src_stride
            elif src_stride is None:
                raise ValueError("set_constants: a flat source needs src_stride")
            if n > 0 and src.size < (n - 1) * int(src_stride) + 1:
                raise ValueError("set_constants: source shorter than the rows it is said to hold")
            if src.size == 0:
                src = np.zeros(1)                    # (n == 0: a valid pointer that is never read)
            ptr, mem = C.c_void_p(src.ctypes.data), MEM_HOST
        _chk(self.L.lpmp_set_constants(self.h, n, factors.ctypes.data, ptr, int(src_stride), mem))

    def zero_pairwise_duals(self):
        """both message vectors of every pairwise factor := +0.0 (lpmp_zero_pairwise_duals)"""
        _chk(self.L.lpmp_zero_pairwise_duals(self.h))

    def schedules_built(self) -> int:
        """schedules, chain plans and joined-pass templates planned and uploaded for the current model since ``upload``"""
        return int(self.L.lpmp_schedules_built(self.h))

    def lower_bound_recomputed(self) -> int:
        """per-factor bounds the last lower_bound() had to recompute (the rest were tracked by the sweep kernels)"""
        return int(self.L.lpmp_lower_bound_recomputed(self.h))

    @property
    def rows_layout(self) -> bool:
        return bool(self.L.lpmp_rows_layout(self.h))

    def table_precision(self) -> str:
        """"f64" / "f32" / "f32_round": how the uploaded model's dense tables are stored (lpmp_table_precision)"""
        code = int(self.L.lpmp_table_precision(self.h))
        return next(k for k, v in TABLE_PRECISIONS.items() if v == code)

    @property
    def plan(self) -> Plan:
        return Plan(_handle=self.L.lpmp_engine_plan_mut(self.h), _owner=self)

    def set_reparametrization(self, mode: int):
        _chk(self.L.lpmp_set_reparametrization(self.h, int(mode)))

    def set_reparametrization_type(self, rtype: int):
        """reference --reparametrizationType: 0 shared, 1 residual, 2 partition, 3 overlapping_partition, 4 adaptive"""
        _chk(self.L.lpmp_set_reparametrization_type(self.h, int(rtype)))

    def set_inner_iterations(self, n: int):
        """reference --innerIteration: passes per partition in the partition sweeps (default 5)"""
        _chk(self.L.lpmp_set_inner_iterations(self.h, int(n)))

    def compute_pass(self, n: int = 1):
        _chk(self.L.lpmp_compute_pass(self.h, int(n)))

    def set_speculation(self, max_passes_ahead: int):
        """let compute_pass(1) run up to that many passes ahead of the caller (include/lpmp_engine.h); 0 = off"""
        _chk(self.L.lpmp_set_speculation(self.h, int(max_passes_ahead)))

    def speculation_stats(self) -> dict:
        v = [C.c_int64() for _ in range(4)]
        _chk(self.L.lpmp_speculation_stats(self.h, *[C.addressof(x) for x in v]))
        return dict(zip(("batches", "passes_launched", "passes_used", "rollbacks"), [x.value for x in v]))

    def peer_minima_launches(self) -> int:
        """joined-pass launches in the peer-minima form since the last reset_kernel_timing (lpmp_get_peer_minima_launches)"""
        nq = C.c_int64()
        _chk(self.L.lpmp_get_peer_minima_launches(self.h, C.addressof(nq)))
        return nq.value

    def chain_cache_bytes(self) -> int:
        return self.L.lpmp_chain_cache_bytes(self.h)

    def set_persistent_launches(self, on: bool):
        """chain executor / joined passes as persistent launches (include/lpmp_engine.h): off for an engine whose device is shared
        with other processes — every schedule then runs launch by launch, same results"""
        _chk(self.L.lpmp_set_persistent_launches(self.h, 1 if on else 0))

    @property
    def persistent_launches(self) -> bool:
        return bool(self.L.lpmp_persistent_launches(self.h))

    def prepare_passes(self, n: int):
        """build ahead of time what compute_pass(n) needs that depends on n (outside of a timed region)"""
        _chk(self.L.lpmp_prepare_passes(self.h, int(n)))

    def forward_pass(self):
        _chk(self.L.lpmp_compute_forward_pass(self.h))

    def backward_pass(self):
        _chk(self.L.lpmp_compute_backward_pass(self.h))

    def compute_pass_custom(self, factors, om_off, om, mk_off, mk):
        factors = np.ascontiguousarray(factors, np.int32)
        om_off = np.ascontiguousarray(om_off, np.int64)
        om = np.ascontiguousarray(om, np.float64)
        mk_off = np.ascontiguousarray(mk_off, np.int64)
        mk = np.ascontiguousarray(mk, np.uint8)
        _chk(self.L.lpmp_compute_pass_custom(self.h, factors.shape[0], factors.ctypes.data, om_off.ctypes.data,
                                             om.ctypes.data, mk_off.ctypes.data, mk.ctypes.data))

    def schedule_create(self, factors, om_off, om, mk_off, mk, fuse: bool = False) -> int:
        """Prepare an iterator-range pass (reference LP_MP.h:981-1005) for repeated replay.  ``fuse``: the list
        concatenates several sweeps; back-to-back updates of one factor are folded into one record."""
        factors = np.ascontiguousarray(factors, np.int32)
        om_off = np.ascontiguousarray(om_off, np.int64)
        om = np.ascontiguousarray(om, np.float64)
        mk_off = np.ascontiguousarray(mk_off, np.int64)
        mk = np.ascontiguousarray(mk, np.uint8)
        sid = C.c_int()
        _chk(self.L.lpmp_schedule_create_fused(self.h, factors.shape[0], factors.ctypes.data, om_off.ctypes.data,
                                               om.ctypes.data, mk_off.ctypes.data, mk.ctypes.data, 1 if fuse else 0,
                                               C.addressof(sid)))
        return sid.value

    def schedule_run(self, sid: int):
        _chk(self.L.lpmp_schedule_run(self.h, int(sid)))

    def schedule_info(self, sid: int) -> dict:
        v = [C.c_int64() for _ in range(5)]
        _chk(self.L.lpmp_schedule_info(self.h, int(sid), *[C.addressof(x) for x in v]))
        return dict(zip(("n_levels", "n_launches", "n_receives", "n_sends", "algorithmic_bytes"), [x.value for x in v]))

    def schedule_destroy(self, sid: int):
        _chk(self.L.lpmp_schedule_destroy(self.h, int(sid)))

    def lower_bound(self, dst_dev: Optional[int] = None):
        """LP::LowerBound.  ``dst_dev``: a raw device pointer to one double — the value is written there asynchronously on the
        engine's stream, without any host synchronisation (lpmp_lower_bound_dev), and the call returns None"""
        if dst_dev is not None:
            _chk(self.L.lpmp_lower_bound_dev(self.h, C.c_void_p(dst_dev)))
            return None
        out = C.c_double()
        _chk(self.L.lpmp_lower_bound(self.h, C.addressof(out)))
        return out.value

    # ---- primal rounding inside the sweep (reference LP_MP.h:914-940, 1067-1082, 1521-1536) ----
    def forward_pass_and_primal(self, iteration: int):
        _chk(self.L.lpmp_compute_forward_pass_and_primal(self.h, int(iteration)))

    def backward_pass_and_primal(self, iteration: int):
        _chk(self.L.lpmp_compute_backward_pass_and_primal(self.h, int(iteration)))

    def compute_pass_and_primal(self, iteration: int):
        _chk(self.L.lpmp_compute_pass_and_primal(self.h, int(iteration)))

    def decode_primal(self, direction: int = 0, refine: int = 0):
        """labels from the current duals by conditional rounding (lpmp_decode_primal): every unary, in the order of
        ``direction`` (0 forward, 1 backward), takes the first minimiser of its reparametrised cost given the labels of the
        neighbours already visited; then ``refine`` sweeps in which every neighbour counts (ICM on the original energy).  Reads the
        duals only; the labels land where ``download_primal`` / ``evaluate_primal`` read them.  Decode against the direction of
        the last sweep: forward after ``compute_pass``."""
        _chk(self.L.lpmp_decode_primal(self.h, int(direction), int(refine)))

    def readout(self, factors=None) -> "Readout":
        """a prepared read-out of the listed VECTOR factors (lpmp_readout_create; None: every VECTOR factor in ascending index):
        labels, unaries and beliefs into device or host arrays without planning or uploading anything per call"""
        return Readout(self, factors)

    def window_set(self, factors=None) -> "WindowSet":
        """a prepared set of VECTOR factors whose label windows move together (lpmp_window_set_create; None: every VECTOR factor):
        ``WindowSet.move`` carries their unaries, their messages and the shifts of the adjacent DIFF_SHIFT factors along"""
        return WindowSet(self, factors)

    def path_set(self, groups) -> "PathSet":
        """a prepared set of paths of VECTOR factors (lpmp_path_set_create): ``groups`` is a sequence of groups, each a sequence of
        paths, each a sequence of factor indices whose consecutive members share exactly one pairwise factor.  ``PathSet.move``
        relabels every path exactly, given all other labels"""
        return PathSet(self, groups)

    def forest_set(self, groups) -> "ForestSet":
        """a prepared set of forests of VECTOR factors (lpmp_forest_set_create): ``groups`` is a sequence of (unaries, parent) pairs
        — parent[i] the factor index of the parent of unaries[i], -1 for a root — whose members induce a forest;
        ``Plan.suggest_forests`` covers any model with such groups, ``model.forests_from_paths`` turns path groups into them.
        ``ForestSet.move`` relabels every tree exactly, given all other labels"""
        return ForestSet(self, groups)

    def check_primal_consistency(self) -> bool:
        out = C.c_int()
        _chk(self.L.lpmp_check_primal_consistency(self.h, C.addressof(out)))
        return bool(out.value)

    def evaluate_primal(self, dst_dev: Optional[int] = None):
        """LP::EvaluatePrimal (+inf when inconsistent / unset).  ``dst_dev``: a raw device pointer to one double — written
        asynchronously on the engine's stream without any host synchronisation (lpmp_evaluate_primal_dev); returns None"""
        if dst_dev is not None:
            _chk(self.L.lpmp_evaluate_primal_dev(self.h, C.c_void_p(dst_dev)))
            return None
        out = C.c_double()
        _chk(self.L.lpmp_evaluate_primal(self.h, C.addressof(out)))
        return out.value

    def download_primal(self) -> np.ndarray:
        """[n_factors, 2] primal_ members: vector (label, 0), pairwise (x0, x1); unset = the dimension"""
        out = np.empty((self.model.n_factors, 2), np.int32)
        _chk(self.L.lpmp_download_primal(self.h, out.ctypes.data))
        return out

    def upload_primal(self, primal: np.ndarray):
        primal = np.ascontiguousarray(primal, np.int32)
        assert primal.shape == (self.model.n_factors, 2)
        _chk(self.L.lpmp_upload_primal(self.h, primal.ctypes.data))

    def factor_lower_bounds(self) -> np.ndarray:
        out = np.empty(self.model.n_factors, np.float64)
        _chk(self.L.lpmp_factor_lower_bounds(self.h, out.ctypes.data))
        return out

    def invalidate_lower_bounds(self):
        """duals were changed outside the engine (borrowed buffer): recompute every factor's bound next time"""
        _chk(self.L.lpmp_invalidate_lower_bounds(self.h))

    def synchronize(self):
        _chk(self.L.lpmp_synchronize(self.h))

    def download_duals(self) -> np.ndarray:
        out = np.empty(self.L.lpmp_dual_size(self.h), np.float64)
        _chk(self.L.lpmp_download_duals(self.h, out.ctypes.data))
        return out

    def upload_duals(self, d: np.ndarray):
        d = np.ascontiguousarray(d, np.float64)
        assert d.shape[0] == self.L.lpmp_dual_size(self.h)
        _chk(self.L.lpmp_upload_duals(self.h, d.ctypes.data))

    def device_duals_ptr(self) -> int:
        return self.L.lpmp_device_duals(self.h)

    # ---- boundary step of the partitioned sweep (include/lpmp_engine.h, csrc/boundary.hip) ----
    def boundary_create(self, out_dual_off, out_len, in_dual_off, in_len, in_omega, in_order) -> int:
        a = [np.ascontiguousarray(out_dual_off, np.int64), np.ascontiguousarray(out_len, np.int32),
             np.ascontiguousarray(in_dual_off, np.int64), np.ascontiguousarray(in_len, np.int32),
             np.ascontiguousarray(in_omega, np.float64), np.ascontiguousarray(in_order, np.int64)]
        h = C.c_void_p()
        _chk(self.L.lpmp_boundary_create(self.h, a[0].shape[0], a[0].ctypes.data, a[1].ctypes.data, a[2].shape[0],
                                         a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data, a[5].ctypes.data, C.addressof(h)))
        return h.value

    def boundary_destroy(self, b: int):
        self.L.lpmp_boundary_destroy(b)

    def boundary_sizes(self, b: int):
        return self.L.lpmp_boundary_out_doubles(b), self.L.lpmp_boundary_in_doubles(b)

    def boundary_pack(self, b: int, send_ptr: int):
        _chk(self.L.lpmp_boundary_pack(self.h, b, C.c_void_p(send_ptr)))

    def boundary_reply(self, b: int, recv_ptr: int, reply_ptr: int):
        _chk(self.L.lpmp_boundary_reply(self.h, b, C.c_void_p(recv_ptr), C.c_void_p(reply_ptr)))

    def boundary_fold(self, b: int, back_ptr: int):
        _chk(self.L.lpmp_boundary_fold(self.h, b, C.c_void_p(back_ptr)))

    # ---- halos of the lock-step sweep (csrc/boundary.hip): vectors as (packed dual offset, length), exchange order ----
    def halo_create(self, out_dual_off, out_len, in_dual_off, in_len) -> int:
        a = [np.ascontiguousarray(out_dual_off, np.int64), np.ascontiguousarray(out_len, np.int32),
             np.ascontiguousarray(in_dual_off, np.int64), np.ascontiguousarray(in_len, np.int32)]
        h = C.c_void_p()
        _chk(self.L.lpmp_halo_create(self.h, a[0].shape[0], a[0].ctypes.data, a[1].ctypes.data, a[2].shape[0], a[2].ctypes.data,
                                     a[3].ctypes.data, C.addressof(h)))
        return h.value

    def halo_destroy(self, h: int):
        self.L.lpmp_halo_destroy(h)

    def halo_sizes(self, h: int):
        return self.L.lpmp_halo_out_doubles(h), self.L.lpmp_halo_in_doubles(h)

    def halo_pack(self, h: int, send_ptr: int):
        _chk(self.L.lpmp_halo_pack(self.h, h, C.c_void_p(send_ptr)))

    def halo_unpack(self, h: int, recv_ptr: int):
        _chk(self.L.lpmp_halo_unpack(self.h, h, C.c_void_p(recv_ptr)))

    def enable_kernel_timing(self, on: bool):
        _chk(self.L.lpmp_enable_kernel_timing(self.h, 1 if on else 0))

    def reset_kernel_timing(self):
        _chk(self.L.lpmp_reset_kernel_timing(self.h))

    def kernel_timing(self) -> dict:
        ms = np.zeros(N_KCLASS, np.float64)
        arrs = [np.zeros(N_KCLASS, np.int64) for _ in range(4)]
        _chk(self.L.lpmp_get_kernel_timing(self.h, N_KCLASS, ms.ctypes.data, *[a.ctypes.data for a in arrs]))
        chain = np.zeros(N_KCLASS, np.int64)
        _chk(self.L.lpmp_get_chain_launches(self.h, N_KCLASS, chain.ctypes.data))
        out = {}
        f32 = hasattr(self.L, "lpmp_table_precision") and int(self.L.lpmp_table_precision(self.h)) != TABLES_F64
        for c in range(N_KCLASS):
            if arrs[0][c] > 0:
                name = KERNEL_NAMES[c]
                if f32 and c in _F32_KERNEL_CLASSES:     # float tables: the kernels of their own the launch wrappers select
                    name = name.replace("_kernel", "_f32_kernel")
                if chain[c] > 0:             # joined passes as persistent launches: plain table loads, agent-scope dual accesses
                    name = name.replace("sweep_", "chain_")
                    if not name.endswith(">") and "dense" in name:
                        name += ", false>"
                    elif not name.endswith(">"):
                        name += ">"
                    out[KCLASS_NAMES[c]] = dict(kernel=name, ms=float(ms[c]), launches=int(arrs[0][c]), chain_launches=int(chain[c]),
                                                factors=int(arrs[1][c]), receives=int(arrs[2][c]), bytes=int(arrs[3][c]))
                    if KCLASS_NAMES[c] == "dense32" and hasattr(self.L, "lpmp_get_peer_minima_launches"):
                        # joined passes in the peer-minima form; the kernel string stays the class's
                        nq = C.c_int64()
                        _chk(self.L.lpmp_get_peer_minima_launches(self.h, C.addressof(nq)))
                        out[KCLASS_NAMES[c]]["peer_minima_launches"] = nq.value
                    continue
                if not name.endswith(">") and "<" in name:       # exact dense kernels: plain / non-temporal form
                    name += ", true>" if self.L.lpmp_streaming_access(self.h) == 1 else ", false>"
                elif name in ("sweep_dense_big_kernel", "sweep_dense_big_f32_kernel"):
                    name += "<true>" if self.L.lpmp_streaming_access(self.h) == 1 else "<false>"
                out[KCLASS_NAMES[c]] = dict(kernel=name, ms=float(ms[c]), launches=int(arrs[0][c]),
                                            factors=int(arrs[1][c]), receives=int(arrs[2][c]), bytes=int(arrs[3][c]))
                if name == "sweep_diff_kernel" and hasattr(self.L, "lpmp_get_diff_band_launches"):
                    # launches whose vectors are all banded run the banded kernel; the name is its only when all timed ones did
                    nb = C.c_int64()
                    _chk(self.L.lpmp_get_diff_band_launches(self.h, C.addressof(nb)))
                    out[KCLASS_NAMES[c]]["band_launches"] = nb.value
                    if nb.value == arrs[0][c]:
                        out[KCLASS_NAMES[c]]["kernel"] = "sweep_diff_band_kernel"
                    if hasattr(self.L, "lpmp_get_diff_shift_launches"):
                        # launches that touch a DIFF_SHIFT factor run one of the two shifted kernels; the name as above, whichever
                        # of them ran: shift_band_launches tells sweep_diff_shift_band_kernel from sweep_diff_shift_kernel
                        ns = C.c_int64()
                        _chk(self.L.lpmp_get_diff_shift_launches(self.h, C.addressof(ns)))
                        out[KCLASS_NAMES[c]]["shift_launches"] = ns.value
                        if ns.value == arrs[0][c]:
                            out[KCLASS_NAMES[c]]["kernel"] = "sweep_diff_shift_kernel"
                        if hasattr(self.L, "lpmp_get_diff_shift_band_launches"):
                            nsb = C.c_int64()
                            _chk(self.L.lpmp_get_diff_shift_band_launches(self.h, C.addressof(nsb)))
                            out[KCLASS_NAMES[c]]["shift_band_launches"] = nsb.value
        return out


class _PreparedSet:
    """What the four prepared sets share: the engine and library handles, the handle the library's create call returns, and
    ``close`` / ``__del__`` through the library call that ``_destroy`` names."""
    _destroy = None

    def _create(self, engine: Engine, create: str, *args):
        self.e = engine
        self.L = engine.L
        h = C.c_void_p()
        _chk(getattr(self.L, create)(engine.h, *args, C.addressof(h)))
        self.h = h.value

    def _create_listed(self, engine: Engine, create: str, factors):
        """a set made from a list of factors, or from None: every VECTOR factor"""
        if factors is None:
            self._create(engine, create, 0, None)
        else:
            factors = np.ascontiguousarray(factors, np.int32).reshape(-1)
            self._create(engine, create, int(factors.shape[0]), _valid_ptr(factors).ctypes.data)

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _int32_list(values, n: int, who: str, noun: str):
    """``values`` (None: an empty list) as ``n`` contiguous int32 entries, never an empty array (still a valid pointer)"""
    v = np.asarray([] if values is None else values).reshape(-1)
    if v.shape[0] != n:
        raise ValueError(f"{who}: {n} {noun}s expected, got {v.shape[0]}")
    if n and not np.issubdtype(v.dtype, np.integer):
        raise ValueError(f"{who}: integer {noun}s are expected")
    if n and (v.min() < -(1 << 31) or v.max() >= (1 << 31)):
        raise ValueError(f"{who}: a {noun} does not fit an int32")
    return np.ascontiguousarray(v, np.int32) if n else np.zeros(1, np.int32)


class Readout(_PreparedSet):
    """A prepared list of VECTOR factors of the engine's uploaded model (include/lpmp_engine.h, lpmp_readout_*).  Structure: it stays
    valid across new costs, passes and decodes; after the engine's next ``upload`` every call raises (LPMP_ERR_STATE) and ``close``
    still works.  ``dst_dev``: a raw device pointer — the call is asynchronous on the engine's stream and returns None."""
    _destroy = "lpmp_readout_destroy"

    def __init__(self, engine: Engine, factors=None):
        self._create_listed(engine, "lpmp_readout_create", factors)
        self.n = int(self.L.lpmp_readout_n(self.h))
        self.max_labels = int(self.L.lpmp_readout_max_labels(self.h))

    def labels(self, dst_dev: Optional[int] = None):
        """[n] int32: the label slot of every listed factor as ``Engine.download_primal`` reports it (unset: the label count)"""
        if dst_dev is not None:
            _chk(self.L.lpmp_readout_labels(self.e.h, self.h, C.c_void_p(dst_dev), MEM_DEVICE))
            return None
        out = np.zeros(max(self.n, 1), np.int32)
        _chk(self.L.lpmp_readout_labels(self.e.h, self.h, out.ctypes.data, MEM_HOST))
        return out[:self.n]

    def set_labels(self, src=None, src_dev: Optional[int] = None):
        """the input twin of ``labels`` (lpmp_readout_set_labels): ``src`` an integer array of ``n`` entries, entry i the label of
        listed factor i, its label count meaning unset; or ``src_dev`` a raw device pointer to int32 values (asynchronous on the
        engine's stream; values that are no label are stored as unset).  A read-out that lists a factor twice is refused."""
        if src_dev is not None:
            _chk(self.L.lpmp_readout_set_labels(self.e.h, self.h, C.c_void_p(src_dev), MEM_DEVICE))
            return
        s = _int32_list(src, self.n, "set_labels", "label")
        _chk(self.L.lpmp_readout_set_labels(self.e.h, self.h, C.c_void_p(s.ctypes.data), MEM_HOST))

    def _rows(self, fn, dst_dev, stride):
        stride = self.max_labels if stride is None else int(stride)
        if dst_dev is not None:
            _chk(fn(self.e.h, self.h, C.c_void_p(dst_dev), stride, MEM_DEVICE))
            return None
        out = np.full(max(self.n * max(stride, 0), 1), np.nan)
        _chk(fn(self.e.h, self.h, out.ctypes.data, stride, MEM_HOST))
        return out[:self.n * stride].reshape(self.n, stride)

    def vectors(self, dst_dev: Optional[int] = None, stride: Optional[int] = None):
        """[n, stride] float64: row i is the current theta of listed factor i; entries beyond its label count are NaN (a device
        destination keeps what it held there)"""
        return self._rows(self.L.lpmp_readout_vectors, dst_dev, stride)

    def beliefs(self, dst_dev: Optional[int] = None, stride: Optional[int] = None):
        """[n, stride] float64: row i is the belief of listed factor i — theta plus what every adjacent pairwise factor would send it,
        in the order of its message list (include/lpmp_engine.h has the rule); padding as in ``vectors``"""
        return self._rows(self.L.lpmp_readout_beliefs, dst_dev, stride)


class WindowSet(_PreparedSet):
    """A prepared list of distinct VECTOR factors of the engine's uploaded model whose label windows move together
    (include/lpmp_engine.h, lpmp_window_set_* / lpmp_move_windows).  Structure, like a ``Readout``: it stays valid across new costs,
    passes and moves; after the engine's next ``upload`` every move raises (LPMP_ERR_STATE) and ``close`` still works."""
    _destroy = "lpmp_window_set_destroy"

    def __init__(self, engine: Engine, factors=None):
        self._create_listed(engine, "lpmp_window_set_create", factors)
        self.n = int(self.L.lpmp_window_set_n(self.h))
        self.n_pairwise = int(self.L.lpmp_window_set_n_pairwise(self.h))
        self.max_labels = int(self.L.lpmp_window_set_max_labels(self.h))

    def move(self, delta=None, delta_dev: Optional[int] = None, cost_old=None, cost_new=None, cost_dev=None, stride: Optional[int] = None,
             carry_labels: bool = False):
        """move the window of listed factor i by ``delta[i]`` labels (lpmp_move_windows): ``delta`` an integer array of ``n`` entries
        with |delta| <= 2^20, or ``delta_dev`` a raw device pointer to int32 values.  ``cost_old`` / ``cost_new``: the original unary
        costs in the old and in the new window as [n, >= max_labels] arrays (both or neither), or ``cost_dev=(old_ptr, new_ptr)`` raw
        device pointers with ``stride``; a pointer of the pair may be None to hand the library one array alone (refused).  With
        device inputs only the call is asynchronous on the engine's stream.  ``Engine.model`` keeps the constants of the upload
        (``model.move_windows`` gives the moved model; ``LP.move_windows`` keeps the mirror's books).
        ``carry_labels``: the labels move with their windows instead of becoming unset (lpmp_move_windows_carry;
        ``model.move_labels`` is the numpy statement)."""
        if delta_dev is not None:
            dp, dm = C.c_void_p(delta_dev), MEM_DEVICE
        else:
            d = _int32_list(delta, self.n, "move", "delta")
            dp, dm = C.c_void_p(d.ctypes.data), MEM_HOST
        co = cn = None
        cm, cs = MEM_HOST, 0
        if cost_dev is not None:
            if stride is None:
                raise ValueError("move: cost_dev needs stride")
            co, cn = [None if p is None else C.c_void_p(p) for p in cost_dev]
            cm, cs = MEM_DEVICE, int(stride)
        elif cost_old is not None or cost_new is not None:
            arrs = []
            for a in (cost_old, cost_new):
                if a is None:
                    arrs.append(None)
                    continue
                a = np.ascontiguousarray(a, np.float64)
                if a.ndim != 2 or a.shape[0] < self.n:
                    raise ValueError("move: costs are [n, >= max_labels] arrays")
                arrs.append(a)
            have = [a for a in arrs if a is not None]
            if len(have) == 2 and have[0].shape != have[1].shape:
                raise ValueError("move: cost_old and cost_new differ in shape")
            cs = int(have[0].shape[1]) if stride is None else int(stride)
            if cs > have[0].shape[1]:
                raise ValueError("move: stride beyond the rows of the cost arrays")
            co, cn = [None if a is None else C.c_void_p(a.ctypes.data) for a in arrs]
        fn = self.L.lpmp_move_windows_carry if carry_labels else self.L.lpmp_move_windows
        _chk(fn(self.e.h, self.h, dp, dm, co, cn, cs, cm))


class PathSet(_PreparedSet):
    """Prepared groups of paths of the engine's uploaded model (include/lpmp_engine.h, lpmp_path_set_* / lpmp_path_moves).  Structure,
    like a ``Readout``: it stays valid across new costs, passes, decodes and window moves; after the engine's next ``upload`` every
    move raises (LPMP_ERR_STATE) and ``close`` still works."""
    _destroy = "lpmp_path_set_destroy"

    def __init__(self, engine: Engine, groups):
        go, po, un = flatten_path_groups(groups)
        self._create(engine, "lpmp_path_set_create", int(go.shape[0]) - 1, go.ctypes.data, po.ctypes.data, _valid_ptr(un).ctypes.data)
        self.n_groups = int(self.L.lpmp_path_set_n_groups(self.h))
        self.n_paths = int(self.L.lpmp_path_set_n_paths(self.h))
        self.longest = int(self.L.lpmp_path_set_longest(self.h))
        self.scratch_bytes = int(self.L.lpmp_path_set_scratch_bytes(self.h))

    def move(self, rounds: int = 1):
        """``rounds`` times over the groups in their order: every path takes the labels that minimise the energy over it given all
        other labels (lpmp_path_moves).  Asynchronous on the engine's stream; reads duals, constants and labels, writes labels."""
        _chk(self.L.lpmp_path_moves(self.e.h, self.h, int(rounds)))


class ForestSet(_PreparedSet):
    """Prepared groups of forests of the engine's uploaded model (include/lpmp_engine.h, lpmp_forest_set_* / lpmp_forest_moves).
    Structure, like a ``PathSet``: it stays valid across new costs, passes, decodes and window moves; after the engine's next
    ``upload`` every move raises (LPMP_ERR_STATE) and ``close`` still works."""
    _destroy = "lpmp_forest_set_destroy"

    def __init__(self, engine: Engine, groups):
        go, un, par = flatten_forest_groups(groups)
        self._create(engine, "lpmp_forest_set_create", int(go.shape[0]) - 1, go.ctypes.data, _valid_ptr(un).ctypes.data, _valid_ptr(par).ctypes.data)
        self.n_groups = int(self.L.lpmp_forest_set_n_groups(self.h))
        self.n_trees = int(self.L.lpmp_forest_set_n_trees(self.h))
        self.max_height = int(self.L.lpmp_forest_set_max_height(self.h))
        self.scratch_bytes = int(self.L.lpmp_forest_set_scratch_bytes(self.h))

    def move(self, rounds: int = 1):
        """``rounds`` times over the groups in their order: every tree takes the labels that minimise the energy over it given all
        other labels (lpmp_forest_moves).  Asynchronous on the engine's stream; reads duals, constants and labels, writes labels."""
        _chk(self.L.lpmp_forest_moves(self.e.h, self.h, int(rounds)))


def device_identity(device: int = 0) -> str:
    """"pci=... uuid=..." of a HIP device ordinal: equal strings = one physical GPU, whatever each process calls it"""
    buf = C.create_string_buffer(128)
    _chk(lib().lpmp_device_identity(int(device), buf, 128))
    return buf.value.decode()


def synth_fill_blocks(device_ptr: int, n_blocks: int, block_len: int, seed: int, first_dev_ptr: int, stream_ptr: int = 0):
    """block b of ``block_len`` values continues the global u01 stream at first[b] (int64 device array)"""
    _chk(lib().lpmp_synth_fill_blocks(C.c_void_p(device_ptr), n_blocks, block_len, C.c_uint64(seed), C.c_void_p(first_dev_ptr), C.c_void_p(stream_ptr)))


def synth_fill(device_ptr: int, n: int, seed: int, first: int = 0, stream_ptr: int = 0):
    _chk(lib().lpmp_synth_fill(C.c_void_p(device_ptr), n, C.c_uint64(seed), C.c_uint64(first), C.c_void_p(stream_ptr)))
