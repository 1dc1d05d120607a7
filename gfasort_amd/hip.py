"""ctypes binding of libgfasort_hip.so (include/gfasort_hip.h).  There is no CPU fallback:
if the library is missing this module raises, and compute calls on a machine without a HIP
device return GFS_E_HIP (raised as GfsError)."""
import ctypes as C
import os

import numpy as np

from . import build as _build
from .quality import sort_quality_figures

NO_NODE = 0xFFFFFFFF
MAX_DIMS = 8
OK, NOTHING_TO_DO = 0, 1
F_PLAIN_LOADS, F_NO_LDS_TABLES, F_NO_FUSE = 1, 2, 4


F_DBG_NO_ATOMICS, F_DBG_NO_XLOADS, F_DBG_ONE_COLOUR = 0x100, 0x200, 0x800
F_DBG_NO_ALIGN, F_DBG_ALIGN_FIRST, F_DBG_WIDE_INDEX, F_DBG_NO_FUSED_TRIP = 0x1000, 0x2000, 0x4000, 0x8000
F_ONE_PARTNER, F_DBG_NO_TWIN_TRIP, F_DBG_FREE_RUNNING = 0x10, 0x400, 0x20
F_FULL_RECORDS = 0x80      # GFS_F_FULL_RECORDS: the 1D team kernels' trips read 16-byte step records even where 8-byte trip records would do
F_PHASED = 0x40            # GFS_F_PHASED: the 1D sort's phased sampler (reference streams in a window of iterations)


def F_CHAIN(k):
    """GFS_F_CHAIN(k): longest run in trips at B = 64 (0 = auto: 64 for the 1D sort, 16 for layouts; else a power of two <= 64)."""
    return (int(k) & 0xFF) << 24


def F_BUNDLE(n):
    """GFS_F_BUNDLE(n): 0 = auto, 1 = reference streams, 4..64 = explicit bundle width."""
    return (int(n) & 0xFF) << 16


class GfsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gfasort_hip error {code}: {msg}")
        self.code = code


class GraphView(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_steps", C.c_uint64), ("n_paths", C.c_uint64),
                ("node_len", C.c_void_p), ("step_node", C.c_void_p),
                ("step_is_rev", C.c_void_p), ("path_first_step", C.c_void_p)]


class SgdParams(C.Structure):
    _fields_ = [("iter_max", C.c_uint64), ("iter_with_max_learning_rate", C.c_uint64),
                ("min_term_updates", C.c_uint64), ("delta", C.c_double), ("eps", C.c_double),
                ("eta_max", C.c_double), ("theta", C.c_double), ("space", C.c_uint64),
                ("space_max", C.c_uint64), ("space_quantization_step", C.c_uint64),
                ("cooling_start", C.c_double), ("nthreads", C.c_uint64),
                ("progress", C.c_uint8), ("_pad", C.c_uint8 * 7), ("seed", C.c_uint64)]


class LayoutParams(C.Structure):
    _fields_ = [("dimensions", C.c_uint64), ("sgd", SgdParams)]


class LaunchConfig(C.Structure):
    _fields_ = [("n_streams", C.c_uint64), ("stream_base", C.c_uint64),
                ("term_updates_per_iteration", C.c_uint64), ("attempt_factor", C.c_uint64),
                ("block_size", C.c_uint32), ("flags", C.c_uint32), ("trace_per_stream", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("term_updates", C.c_uint64), ("attempts", C.c_uint64), ("iterations", C.c_uint64),
                ("n_streams", C.c_uint64), ("bundle", C.c_uint64), ("kernel_ms", C.c_double),
                ("total_ms", C.c_double), ("launches", C.c_uint64), ("run_trips", C.c_uint64)]


class RankConfig(C.Structure):
    _fields_ = [("rank", C.c_uint32), ("world", C.c_uint32), ("device", C.c_int32), ("sharding", C.c_uint32),
                ("merge_every", C.c_uint32), ("merge_rule", C.c_uint32), ("payload", C.c_uint32), ("exchange", C.c_uint32),
                ("launch", LaunchConfig)]


class RankInfo(C.Structure):
    _fields_ = [("quota", C.c_uint64), ("shard_steps", C.c_uint64), ("span_lo", C.c_uint64), ("span_hi", C.c_uint64),
                ("shared_slots", C.c_uint64), ("exchange_count", C.c_uint64), ("positions_len", C.c_uint64),
                ("windows", C.c_uint64), ("last_merge_kernels_ms", C.c_double), ("idle", C.c_uint32), ("_pad", C.c_uint32)]


class PairError(C.Structure):
    """gfs_pair_error: all pairs of steps (s, s + step_distance) of one path."""
    _fields_ = [("step_distance", C.c_uint64), ("pairs", C.c_uint64), ("sum_rel_sq", C.c_double), ("max_rel_sq", C.c_double),
                ("sum_abs", C.c_double), ("sum_sq", C.c_double)]


class SortQuality(C.Structure):
    """gfs_sort_quality: measure_layout_quality.rs on the graph sorted by the current 1D positions."""
    _fields_ = [("steps", C.c_uint64), ("abs_err_sum", C.c_uint64), ("genomic_sum", C.c_uint64), ("sq_err_sum", C.c_double)]


class BatchConfig(C.Structure):
    """gfs_batch_config."""
    _fields_ = [("max_blocks_per_launch", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class BatchStats(C.Structure):
    """gfs_batch_stats: kernel_ms is the batch's (a batch does not advance its contexts' kernel_ms)."""
    _fields_ = [("items", C.c_uint64), ("items_run", C.c_uint64), ("launches", C.c_uint64), ("blocks", C.c_uint64),
                ("term_updates", C.c_uint64), ("attempts", C.c_uint64), ("kernel_ms", C.c_double), ("total_ms", C.c_double)]


class ContextSetInfo(C.Structure):
    """gfs_ctx_set_info: launches counts the library's own kernels and memsets one by one and each rocPRIM call as one."""
    _fields_ = [("items", C.c_uint64), ("total_nodes", C.c_uint64), ("total_steps", C.c_uint64), ("total_paths", C.c_uint64),
                ("launches", C.c_uint64), ("device_allocations", C.c_uint64), ("arena_bytes", C.c_uint64), ("build_ms", C.c_double)]


class ContextSetSetupInfo(C.Structure):
    """gfs_ctx_set_setup_info: the last gfs_ctx_set_setup_* of a set, counted as ContextSetInfo counts."""
    _fields_ = [("items", C.c_uint64), ("configured", C.c_uint64), ("nothing_to_do", C.c_uint64), ("total_streams", C.c_uint64),
                ("state_bytes", C.c_uint64), ("device_allocations", C.c_uint64), ("copies", C.c_uint64), ("launches", C.c_uint64),
                ("setup_ms", C.c_double)]


# GFS_STATE_*: the state arrays of a set-up context (Context.debug_sgd_state), with the dtype each reads as
STATE_POSITIONS, STATE_COUNTERS, STATE_LEAD, STATE_TRACE, STATE_TRACE_COUNTS, STATE_RNG, STATE_ZETAS, STATE_SCHEDULE = range(8)
STATE_KINDS, STATE_SIZE_OF = 8, 0x100
ITER_CONSTS_DTYPE = np.dtype([("eta", "<f8"), ("zeta2theta", "<f8"), ("omt_fb", "<f8"), ("alpha_fb", "<f8"), ("omt_e", "<i4"),
                              ("alpha_e", "<i4"), ("cooling", "<i4"), ("_pad", "<i4")])

PAIR_ERROR_DTYPE = np.dtype([("step_distance", "<u8"), ("pairs", "<u8"), ("sum_rel_sq", "<f8"), ("max_rel_sq", "<f8"),
                             ("sum_abs", "<f8"), ("sum_sq", "<f8")])

SORT_QUALITY_DTYPE = np.dtype([("steps", "<u8"), ("abs_err_sum", "<u8"), ("genomic_sum", "<u8"), ("sq_err_sum", "<f8")])   # gfs_sort_quality

# gfs_path_error, gfs_stretched_pair, gfs_node_error (K7d, K7e, K7f)
PATH_ERROR_DTYPE = np.dtype([("steps", "<u8"), ("reverse_steps", "<u8"), ("pairs", "<u8"), ("sum_rel_sq", "<f8"), ("max_rel_sq", "<f8"),
                             ("sum_abs", "<f8"), ("sum_sq", "<f8"), ("stretched", "<u8")])
STRETCHED_PAIR_DTYPE = np.dtype([("step_a", "<u8"), ("step_b", "<u8"), ("path", "<u8"), ("d_path", "<f8"), ("d_layout", "<f8")])
NODE_ERROR_DTYPE = np.dtype([("pairs", "<u8"), ("stretched", "<u8"), ("max_rel_sq", "<f8")])

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p)
MERGE_RULES = {"anneal": 0, "sum": 1, "mean": 2, "touch": 3}

TERM_DTYPE = np.dtype([("i", "<u4"), ("j", "<u4"), ("d_ij", "<f8")], align=True)

# every symbol include/gfasort_hip.h declares
EXPORTS = [
    "gfs_version", "gfs_last_error", "gfs_device_count", "gfs_warmup", "gfs_fast_precise_pow", "gfs_sgd_schedule",
    "gfs_zeta_table_len", "gfs_zeta_table", "gfs_init_positions", "gfs_init_layout_dim0", "gfs_init_layout",
    "gfs_sort_order", "gfs_path_linear_sgd", "gfs_path_sgd_sort", "gfs_path_linear_sgd_layout", "gfs_ctx_create",
    "gfs_ctx_create_with_layout", "gfs_ctx_node_layout",
    "gfs_ctx_destroy", "gfs_ctx_setup_1d", "gfs_ctx_setup_nd", "gfs_ctx_positions_len", "gfs_ctx_init_positions",
    "gfs_ctx_upload_positions", "gfs_ctx_download_positions", "gfs_ctx_positions_device",
    "gfs_ctx_bind_positions", "gfs_ctx_reset_streams", "gfs_ctx_run_iteration", "gfs_ctx_run_range", "gfs_ctx_run",
    "gfs_ctx_synchronize", "gfs_ctx_stats", "gfs_ctx_sort_order", "gfs_ctx_trace", "gfs_merge_prepare", "gfs_merge_apply",
    "gfs_shard_paths", "gfs_shard_quotas", "gfs_shared_node_layout", "gfs_exchange_plan",
    "gfs_rank_create", "gfs_rank_destroy", "gfs_rank_ctx", "gfs_rank_get_info", "gfs_rank_set_positions",
    "gfs_rank_positions_changed", "gfs_rank_get_positions", "gfs_rank_exchange_count", "gfs_rank_exchange_buffer",
    "gfs_rank_bind_exchange_buffer", "gfs_rank_window_begin", "gfs_rank_window_end", "gfs_rank_finish_begin",
    "gfs_rank_finish_buffer", "gfs_rank_finish_end", "gfs_rank_run",
    "gfs_ctx_debug_step_records", "gfs_ctx_debug_kshift", "gfs_ctx_record_bytes", "gfs_phase_window", "gfs_ctx_phase_window",
    "gfs_ctx_pair_errors", "gfs_stress_sample_pairs", "gfs_ctx_stress_of_pairs", "gfs_ctx_sort_quality", "gfs_pair_errors",
    "gfs_sort_quality_of", "gfs_batch_sort_quality",
    "gfs_ctx_path_errors", "gfs_ctx_stretched_pairs", "gfs_ctx_node_errors", "gfs_diagnose",
    "gfs_batch_plan", "gfs_batch_create", "gfs_batch_run", "gfs_batch_get_stats", "gfs_batch_destroy",
    "gfs_batch_result_offsets", "gfs_batch_init_positions", "gfs_batch_results", "gfs_batch_debug_sort_cap",
    "gfs_batch_upload_coords", "gfs_batch_coords", "gfs_batch_pair_errors",
    "gfs_batch_path_offsets", "gfs_batch_path_errors", "gfs_batch_stretched_pairs", "gfs_batch_node_errors", "gfs_batch_debug_tile_blocks",
    "gfs_ctx_set_plan", "gfs_ctx_set_create", "gfs_ctx_set_size", "gfs_ctx_set_item", "gfs_ctx_set_get_info", "gfs_ctx_set_destroy",
    "gfs_ctx_set_state_plan", "gfs_ctx_set_setup_1d", "gfs_ctx_set_setup_nd", "gfs_ctx_set_get_setup_info", "gfs_ctx_debug_sgd_state",
]
SEGMENT_SORT_CAP = 8192                # GFS_SEGMENT_SORT_CAP

_lib = None


def lib_path():
    return _build.LIB


def lib():
    """Load libgfasort_hip.so; raises (never falls back) when it is not built."""
    global _lib
    if _lib is None:
        path = os.environ.get("GFS_LIB_PATH") or _build.LIB      # (GFS_LIB_PATH: experiment builds, scripts/ only)
        if not os.path.exists(path):
            raise ImportError(f"{path} is not built: run `python -m gfasort_amd.build` "
                              "(hipcc, gfx950). There is no CPU fallback.")
        L = C.CDLL(path)
        L.gfs_version.restype = C.c_char_p
        L.gfs_last_error.restype = C.c_char_p
        L.gfs_fast_precise_pow.restype = C.c_double
        L.gfs_fast_precise_pow.argtypes = [C.c_double, C.c_double]
        L.gfs_zeta_table_len.restype = C.c_uint64
        L.gfs_ctx_positions_len.restype = C.c_uint64
        L.gfs_ctx_positions_len.argtypes = [C.c_void_p]
        L.gfs_ctx_init_positions.argtypes = [C.c_void_p]
        L.gfs_ctx_positions_device.restype = C.c_void_p
        L.gfs_ctx_positions_device.argtypes = [C.c_void_p]
        L.gfs_ctx_destroy.argtypes = [C.c_void_p]
        L.gfs_ctx_destroy.restype = None
        L.gfs_ctx_run_iteration.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_ctx_run.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_ctx_run_range.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_ctx_synchronize.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_ctx_bind_positions.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_ctx_reset_streams.argtypes = [C.c_void_p]
        L.gfs_ctx_upload_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.gfs_ctx_download_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.gfs_ctx_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_ctx_sort_order.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.gfs_ctx_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        L.gfs_ctx_node_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.gfs_ctx_debug_step_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.gfs_ctx_debug_kshift.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.gfs_ctx_record_bytes.argtypes = [C.c_void_p]
        L.gfs_ctx_record_bytes.restype = C.c_uint32
        L.gfs_phase_window.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gfs_ctx_phase_window.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        L.gfs_ctx_setup_1d.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.gfs_ctx_setup_nd.argtypes = [C.c_void_p] + [C.c_void_p] * 4
        L.gfs_sort_order.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_merge_prepare.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_merge_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_void_p]
        L.gfs_shard_paths.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.gfs_shard_quotas.argtypes = [C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p]
        L.gfs_shared_node_layout.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_exchange_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 9
        L.gfs_rank_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_rank_destroy.argtypes = [C.c_void_p]
        L.gfs_rank_destroy.restype = None
        L.gfs_rank_ctx.argtypes = [C.c_void_p]
        L.gfs_rank_ctx.restype = C.c_void_p
        L.gfs_rank_get_info.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_rank_set_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.gfs_rank_positions_changed.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_rank_get_positions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.gfs_rank_exchange_count.argtypes = [C.c_void_p]
        L.gfs_rank_exchange_count.restype = C.c_uint64
        L.gfs_rank_exchange_buffer.argtypes = [C.c_void_p]
        L.gfs_rank_exchange_buffer.restype = C.c_void_p
        L.gfs_rank_bind_exchange_buffer.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_rank_window_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_rank_window_end.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_rank_finish_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gfs_rank_finish_buffer.argtypes = [C.c_void_p]
        L.gfs_rank_finish_buffer.restype = C.c_void_p
        L.gfs_rank_finish_end.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gfs_rank_run.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p, C.c_void_p]
        L.gfs_ctx_pair_errors.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_stress_sample_pairs.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gfs_ctx_stress_of_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gfs_ctx_sort_quality.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_pair_errors.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_ctx_path_errors.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_ctx_stretched_pairs.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_ctx_node_errors.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_diagnose.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_batch_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_batch_create.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_batch_run.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_batch_get_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_batch_destroy.argtypes = [C.c_void_p]
        L.gfs_batch_destroy.restype = None
        L.gfs_batch_result_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.gfs_batch_init_positions.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_batch_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_batch_debug_sort_cap.argtypes = [C.c_void_p, C.c_uint64]
        L.gfs_batch_upload_coords.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.gfs_batch_coords.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_batch_pair_errors.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gfs_batch_path_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.gfs_batch_path_errors.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_batch_stretched_pairs.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gfs_batch_node_errors.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_batch_debug_tile_blocks.argtypes = [C.c_void_p, C.c_uint64]
        L.gfs_sort_quality_of.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gfs_batch_sort_quality.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_ctx_set_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_ctx_set_create.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
        L.gfs_ctx_set_size.argtypes = [C.c_void_p]
        L.gfs_ctx_set_size.restype = C.c_uint64
        L.gfs_ctx_set_item.argtypes = [C.c_void_p, C.c_uint64]
        L.gfs_ctx_set_item.restype = C.c_void_p
        L.gfs_ctx_set_get_info.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_ctx_set_destroy.argtypes = [C.c_void_p]
        L.gfs_ctx_set_destroy.restype = None
        L.gfs_ctx_set_state_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gfs_ctx_set_setup_1d.argtypes = [C.c_void_p] * 4
        L.gfs_ctx_set_setup_nd.argtypes = [C.c_void_p] * 4
        L.gfs_ctx_set_get_setup_info.argtypes = [C.c_void_p, C.c_void_p]
        L.gfs_ctx_debug_sgd_state.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]
        _lib = L
    return _lib


def check(rc):
    if rc < 0:
        raise GfsError(rc, lib().gfs_last_error().decode())
    return rc


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def make_view(g):
    """gfs_graph_view over a FlatGraph; returns (view, keepalive)."""
    arrs = (np.ascontiguousarray(g.node_len, dtype=np.uint32),
            np.ascontiguousarray(g.step_node, dtype=np.uint32),
            np.ascontiguousarray(g.step_is_rev, dtype=np.uint8),
            np.ascontiguousarray(g.path_first_step, dtype=np.uint64))
    v = GraphView(g.n_nodes, g.n_steps, g.n_paths, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2]), _ptr(arrs[3]))
    return v, arrs


def make_sgd_params(p):
    s = SgdParams()
    for name in ("iter_max", "iter_with_max_learning_rate", "min_term_updates", "delta", "eps", "eta_max",
                 "theta", "space", "space_max", "space_quantization_step", "cooling_start", "nthreads", "seed"):
        setattr(s, name, getattr(p, name))
    s.progress = 1 if p.progress else 0
    return s


def phase_window(p):
    """gfs_phase_window: GFS_F_PHASED's default window (k_begin, k_end) for SGD parameters p (host only)."""
    sp = make_sgd_params(p)
    b, e = C.c_uint64(0), C.c_uint64(0)
    check(lib().gfs_phase_window(C.byref(sp), C.byref(b), C.byref(e)))
    return int(b.value), int(e.value)


def make_layout_params(p):
    lp = LayoutParams()
    lp.dimensions = p.dimensions
    lp.sgd = make_sgd_params(p)
    return lp


def make_config(n_streams=0, stream_base=0, term_updates_per_iteration=0, attempt_factor=0,
                block_size=0, flags=0, trace_per_stream=0):
    return LaunchConfig(n_streams, stream_base, term_updates_per_iteration, attempt_factor,
                        block_size, flags, trace_per_stream)


# ---- host tables -----------------------------------------------------------------------------
def fast_precise_pow(a, b):
    return lib().gfs_fast_precise_pow(a, b)


def sgd_schedule(p):
    sp = make_sgd_params(p)
    etas = np.zeros(p.iter_max + 1, dtype=np.float64)
    check(lib().gfs_sgd_schedule(C.byref(sp), _ptr(etas)))
    return etas


def zeta_table(p):
    sp = make_sgd_params(p)
    n = lib().gfs_zeta_table_len(C.byref(sp))
    z = np.zeros(n, dtype=np.float64)
    check(lib().gfs_zeta_table(C.byref(sp), _ptr(z)))
    return z


def init_positions(g):
    v, keep = make_view(g)
    x = np.zeros(g.n_nodes, dtype=np.float64)
    check(lib().gfs_init_positions(C.byref(v), _ptr(x)))
    return x


def init_layout_dim0(g, dims, coords=None):
    v, keep = make_view(g)
    if coords is None:
        coords = np.zeros(g.n_nodes * 2 * dims, dtype=np.float64)
    check(lib().gfs_init_layout_dim0(C.byref(v), C.c_uint64(dims), _ptr(coords)))
    return coords


def init_layout(g, dims, seed):
    """gfs_init_layout: the reference's whole layout start (dimension 0 + StandardNormal dimensions), Layout order."""
    v, keep = make_view(g)
    coords = np.zeros(g.n_nodes * 2 * dims, dtype=np.float64)
    check(lib().gfs_init_layout(C.byref(v), C.c_uint64(dims), C.c_uint64(seed), _ptr(coords)))
    return coords


def sort_order(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    order = np.zeros(x.shape[0], dtype=np.uint64)
    check(lib().gfs_sort_order(_ptr(x), x.shape[0], _ptr(order)))
    return order


def merge_prepare(x_ptr, x_prev_ptr, buf_ptr, n, stream=None):
    check(lib().gfs_merge_prepare(C.c_void_p(x_ptr), C.c_void_p(x_prev_ptr), C.c_void_p(buf_ptr), C.c_uint64(n),
                                  C.c_void_p(stream or 0)))


def merge_apply(x_ptr, x_prev_ptr, buf_ptr, n, divide_all_by=0.0, stream=None):
    check(lib().gfs_merge_apply(C.c_void_p(x_ptr), C.c_void_p(x_prev_ptr), C.c_void_p(buf_ptr), C.c_uint64(n),
                                C.c_double(divide_all_by), C.c_void_p(stream or 0)))


# ---- quality read-outs (K7) --------------------------------------------------------------------
def stress_sample_pairs(g, samples=10000, seed=12345):
    """gfs_stress_sample_pairs (host only): the step pairs (step_a, step_b) calculate_layout_stress draws, less those its
    data-independent `continue`s drop."""
    v, keep = make_view(g)
    sa, sb = np.zeros(max(samples, 1), dtype=np.uint64), np.zeros(max(samples, 1), dtype=np.uint64)
    n = C.c_uint64(0)
    check(lib().gfs_stress_sample_pairs(C.byref(v), C.c_uint64(samples), C.c_uint64(seed), _ptr(sa), _ptr(sb), C.byref(n)))
    return sa[:n.value].copy(), sb[:n.value].copy()


def pair_errors(g, positions, zs, dims=0):
    """gfs_pair_errors: the exhaustive per-step-distance errors of a finished result (dims = 0: x[n_nodes], else Layout.coords
    order), measured on device 0.  Returns a PAIR_ERROR_DTYPE array, one row per z."""
    v, keep = make_view(g)
    x = np.ascontiguousarray(positions, dtype=np.float64)
    if x.shape[0] != (g.n_nodes * 2 * dims if dims else g.n_nodes):
        raise ValueError("positions length does not match the graph and dims")
    zs = np.ascontiguousarray(zs, dtype=np.uint64)
    out = np.zeros(zs.shape[0], dtype=PAIR_ERROR_DTYPE)
    check(lib().gfs_pair_errors(C.byref(v), C.c_uint64(dims), _ptr(x), _ptr(zs), C.c_uint64(zs.shape[0]), _ptr(out)))
    return out


def sort_quality(g, positions):
    """gfs_sort_quality_of: measure_layout_quality.rs on the graph sorted by a finished result's 1D positions x[n_nodes] (dense
    index), measured on device 0.  The dict Context.sort_quality() returns."""
    v, keep = make_view(g)
    x = np.ascontiguousarray(positions, dtype=np.float64)
    if x.shape[0] != g.n_nodes:
        raise ValueError("positions length does not match the graph")
    q = SortQuality()
    check(lib().gfs_sort_quality_of(C.byref(v), _ptr(x), C.byref(q)))
    return sort_quality_figures(q.steps, q.abs_err_sum, q.genomic_sum, q.sq_err_sum)


def diagnose(g, positions, z=1, ratio=10.0, cap=1024, dims=0):
    """gfs_diagnose: per-path errors and the stretched pairs of a finished result at step distance z, measured on device 0.
    Returns (PATH_ERROR_DTYPE array by path, STRETCHED_PAIR_DTYPE array of the first min(cap, total) stretched pairs, total)."""
    v, keep = make_view(g)
    x = np.ascontiguousarray(positions, dtype=np.float64)
    if x.shape[0] != (g.n_nodes * 2 * dims if dims else g.n_nodes):
        raise ValueError("positions length does not match the graph and dims")
    paths = np.zeros(g.n_paths, dtype=PATH_ERROR_DTYPE)
    pairs = np.zeros(int(cap), dtype=STRETCHED_PAIR_DTYPE)
    total = C.c_uint64(0)
    check(lib().gfs_diagnose(C.byref(v), C.c_uint64(dims), _ptr(x), C.c_uint64(z), C.c_double(ratio), _ptr(paths),
                             _ptr(pairs) if cap else None, C.c_uint64(int(cap)), C.byref(total)))
    return paths, pairs[:min(int(cap), int(total.value))], int(total.value)


# ---- multi-device planning (host only) and the rank object -------------------------------------
class ShardPlan:
    """gfs_shard_paths / gfs_shard_quotas / gfs_shared_node_layout / gfs_exchange_plan of a graph for `world` ranks."""

    def __init__(self, g, min_term_updates, world, sharding=0, whole_vector=False):
        v, keep = make_view(g)
        self.world = world
        self.path_owner = np.zeros(max(g.n_paths, 1), dtype=np.uint32)
        self.rank_steps = np.zeros(world, dtype=np.uint64)
        check(lib().gfs_shard_paths(C.byref(v), world, sharding, _ptr(self.path_owner), _ptr(self.rank_steps)))
        self.path_owner = self.path_owner[:g.n_paths]
        self.quotas = np.zeros(world, dtype=np.uint64)
        check(lib().gfs_shard_quotas(C.c_uint64(int(min_term_updates)), _ptr(self.rank_steps), world, _ptr(self.quotas)))
        self.perm = np.zeros(max(g.n_nodes, 1), dtype=np.uint32)
        check(lib().gfs_shared_node_layout(C.byref(v), _ptr(self.perm)))
        self.perm = self.perm[:g.n_nodes]
        self.span_lo, self.span_hi = np.zeros(world, dtype=np.uint64), np.zeros(world, dtype=np.uint64)
        seg_lo, seg_hi = np.zeros(2 * world, dtype=np.uint64), np.zeros(2 * world, dtype=np.uint64)
        own_lo, own_hi = np.zeros(2 * world + 2, dtype=np.uint64), np.zeros(2 * world + 2, dtype=np.uint64)
        own_rank = np.zeros(2 * world + 2, dtype=np.uint32)
        n_seg, n_own = C.c_uint32(0), C.c_uint32(0)
        po = np.ascontiguousarray(self.path_owner) if g.n_paths else np.zeros(1, dtype=np.uint32)
        pm = np.ascontiguousarray(self.perm) if g.n_nodes else np.zeros(1, dtype=np.uint32)
        check(lib().gfs_exchange_plan(C.byref(v), _ptr(pm), _ptr(po), world, _ptr(self.span_lo), _ptr(self.span_hi),
                                      _ptr(seg_lo), _ptr(seg_hi), C.byref(n_seg), _ptr(own_lo), _ptr(own_hi), _ptr(own_rank),
                                      C.byref(n_own)))
        self.shared = [(int(seg_lo[k]), int(seg_hi[k])) for k in range(n_seg.value)]      # slots two or more ranks can move
        if whole_vector and g.n_nodes:
            self.shared = [(0, g.n_nodes)]
        self.owned = [(int(own_lo[k]), int(own_hi[k]), int(own_rank[k])) for k in range(n_own.value)]

    def paths_of(self, rank):
        return np.flatnonzero(self.path_owner == rank).tolist()


class Rank:
    """gfs_rank: one rank of a multi-device run (its shard's context, the exchange of the shared slots)."""

    def __init__(self, g, p, dims, rank, world, device=0, sharding=0, merge_every=1, merge_rule="anneal", payload_f64=False,
                 whole_vector=False, launch=None):
        self.graph, self.params, self.dims = g, p, dims
        v, self._keep = make_view(g)
        cfg = RankConfig(rank, world, device, sharding, merge_every, MERGE_RULES[merge_rule], 1 if payload_f64 else 0,
                         1 if whole_vector else 0, launch if launch is not None else LaunchConfig())
        self.cfg = cfg
        sp = make_sgd_params(p)
        self._h = C.c_void_p()
        self.rc = check(lib().gfs_rank_create(C.byref(v), C.byref(sp), C.c_uint64(dims), C.byref(cfg), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().gfs_rank_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = RankInfo()
        check(lib().gfs_rank_get_info(self._h, C.byref(out)))
        return out

    def ctx_stats(self):
        st = Stats()
        check(lib().gfs_ctx_stats(C.c_void_p(lib().gfs_rank_ctx(self._h)), C.byref(st)))
        return st

    def reset_streams(self):
        check(lib().gfs_ctx_reset_streams(C.c_void_p(lib().gfs_rank_ctx(self._h))))

    def set_positions(self, x=None):
        if x is None:
            check(lib().gfs_rank_set_positions(self._h, None, 0))
        else:
            x = np.ascontiguousarray(x, dtype=np.float64)
            check(lib().gfs_rank_set_positions(self._h, _ptr(x), x.shape[0]))

    def get_positions(self):
        x = np.zeros(int(self.info().positions_len), dtype=np.float64)
        check(lib().gfs_rank_get_positions(self._h, _ptr(x), x.shape[0]))
        return x

    def exchange_count(self):
        return int(lib().gfs_rank_exchange_count(self._h))

    def bind_exchange_buffer(self, device_ptr):
        check(lib().gfs_rank_bind_exchange_buffer(self._h, C.c_void_p(device_ptr)))

    def window_begin(self, ks, stream=None):
        ks = np.ascontiguousarray(ks, dtype=np.uint64)
        return check(lib().gfs_rank_window_begin(self._h, _ptr(ks), C.c_uint64(ks.shape[0]), C.c_void_p(stream or 0)))

    def window_end(self, stream=None):
        check(lib().gfs_rank_window_end(self._h, C.c_void_p(stream or 0)))

    def finish_begin(self, full_device_ptr, stream=None):
        check(lib().gfs_rank_finish_begin(self._h, C.c_void_p(full_device_ptr), C.c_void_p(stream or 0)))

    def finish_end(self, full_device_ptr, stream=None):
        check(lib().gfs_rank_finish_end(self._h, C.c_void_p(full_device_ptr), C.c_void_p(stream or 0)))

    def run(self, allreduce=None, stream=None):
        """gfs_rank_run with a Python collective: allreduce(device_ptr, count, is_f64, stream) -> None."""
        def tramp(user, buf, count, is_f64, st):
            try:
                allreduce(buf, count, bool(is_f64), st)
                return 0
            except Exception:                                  # never raise through the C frame
                import traceback
                traceback.print_exc()
                return 1
        cb = ALLREDUCE_FN(tramp) if allreduce is not None else C.cast(None, ALLREDUCE_FN)
        return check(lib().gfs_rank_run(self._h, cb, None, C.c_void_p(stream or 0)))


# ---- resident context ------------------------------------------------------------------------
class Context:
    """gfs_ctx: the graph's PathIndex mirror, positions and RNG streams resident in HBM."""

    def __init__(self, g, device=0, node_perm=None, _borrowed=None):
        self._h = C.c_void_p()
        self.graph = g
        self.dims = 0
        self.params = None
        self.cfg = None
        self._owns = _borrowed is None
        if not self._owns:                                     # an item of a ContextSet: the set destroys the handle
            self._h, self._keep = C.c_void_p(_borrowed), None
            return
        v, self._keep = make_view(g)
        if node_perm is not None:
            node_perm = np.ascontiguousarray(node_perm, dtype=np.uint32)
        check(lib().gfs_ctx_create_with_layout(C.byref(v), C.c_int(device), _ptr(node_perm), C.byref(self._h)))

    def close(self):
        if self._h:
            if self._owns:
                lib().gfs_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setup_1d(self, p, cfg=None, etas=None, zetas=None):
        sp = make_sgd_params(p)
        self.params, self.cfg, self.dims = p, cfg, 0
        return check(lib().gfs_ctx_setup_1d(self._h, C.byref(sp), C.byref(cfg) if cfg is not None else None,
                                            _ptr(etas), _ptr(zetas)))

    def setup_nd(self, p, cfg=None, etas=None, zetas=None):
        lp = make_layout_params(p)
        self.params, self.cfg, self.dims = p, cfg, p.dimensions
        return check(lib().gfs_ctx_setup_nd(self._h, C.byref(lp), C.byref(cfg) if cfg is not None else None,
                                            _ptr(etas), _ptr(zetas)))

    def positions_len(self):
        return int(lib().gfs_ctx_positions_len(self._h))

    def node_layout(self):
        """perm[k] = slot of dense node k in the device position vector."""
        perm = np.zeros(self.graph.n_nodes, dtype=np.uint32)
        check(lib().gfs_ctx_node_layout(self._h, _ptr(perm), C.c_uint64(perm.shape[0])))
        return perm

    def upload(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        check(lib().gfs_ctx_upload_positions(self._h, _ptr(x), x.shape[0]))

    def init_positions(self):
        """1D: the reference's initial positions, computed on the device."""
        check(lib().gfs_ctx_init_positions(self._h))

    def download(self):
        x = np.zeros(self.positions_len(), dtype=np.float64)
        check(lib().gfs_ctx_download_positions(self._h, _ptr(x), x.shape[0]))
        return x

    def positions_device(self):
        return lib().gfs_ctx_positions_device(self._h)

    def bind_positions(self, device_ptr):
        check(lib().gfs_ctx_bind_positions(self._h, C.c_void_p(device_ptr)))

    def reset_streams(self):
        check(lib().gfs_ctx_reset_streams(self._h))

    def run_iteration(self, k, stream=None):
        return check(lib().gfs_ctx_run_iteration(self._h, C.c_uint64(k), C.c_void_p(stream or 0)))

    def run_range(self, ks, stream=None):
        """Iterations ks (a fused persistent launch where possible)."""
        ks = np.ascontiguousarray(ks, dtype=np.uint64)
        return check(lib().gfs_ctx_run_range(self._h, _ptr(ks), C.c_uint64(ks.shape[0]), C.c_void_p(stream or 0)))

    def run(self, stream=None):
        return check(lib().gfs_ctx_run(self._h, C.c_void_p(stream or 0)))

    def synchronize(self, stream=None):
        check(lib().gfs_ctx_synchronize(self._h, C.c_void_p(stream or 0)))

    def stats(self):
        st = Stats()
        check(lib().gfs_ctx_stats(self._h, C.byref(st)))
        return st

    def sort_order(self):
        """Rank order of the current 1D positions, sorted on the device."""
        order = np.zeros(self.graph.n_nodes, dtype=np.uint64)
        check(lib().gfs_ctx_sort_order(self._h, _ptr(order), C.c_uint64(order.shape[0])))
        return order

    def trace(self):
        st = self.stats()
        k = int(self.cfg.trace_per_stream)
        T = int(st.n_streams)
        out = np.zeros(T * k, dtype=TERM_DTYPE)
        counts = np.zeros(T, dtype=np.uint64)
        check(lib().gfs_ctx_trace(self._h, _ptr(out), T * k, _ptr(counts), T))
        return out.reshape(T, k), counts

    # ---- quality read-outs of the resident positions (K7): nothing is downloaded, nothing is disturbed ----
    def pair_errors(self, zs, stream=None):
        """gfs_ctx_pair_errors: all pairs of steps (s, s + z) for every z of zs.  PAIR_ERROR_DTYPE array, one row per z."""
        zs = np.ascontiguousarray(zs, dtype=np.uint64)
        out = np.zeros(zs.shape[0], dtype=PAIR_ERROR_DTYPE)
        check(lib().gfs_ctx_pair_errors(self._h, _ptr(zs), C.c_uint64(zs.shape[0]), _ptr(out), C.c_void_p(stream or 0)))
        return out

    def stress_of_pairs(self, step_a, step_b):
        """gfs_ctx_stress_of_pairs.  Returns (stress, counted, rel_sq[n]) — rel_sq < 0 marks a skipped pair."""
        sa = np.ascontiguousarray(step_a, dtype=np.uint64)
        sb = np.ascontiguousarray(step_b, dtype=np.uint64)
        if sa.shape != sb.shape:
            raise ValueError("step_a and step_b differ in length")
        rel = np.zeros(sa.shape[0], dtype=np.float64)
        counted, stress = C.c_uint64(0), C.c_double(0.0)
        check(lib().gfs_ctx_stress_of_pairs(self._h, _ptr(sa), _ptr(sb), C.c_uint64(sa.shape[0]), _ptr(rel), C.byref(counted),
                                            C.byref(stress)))
        return float(stress.value), int(counted.value), rel

    def sampled_stress(self, samples=10000, seed=12345):
        """calculate_layout_stress (sgd.rs:1196-1283) of the resident positions: the reference's sample stream, the pairs evaluated
        on the device, summed in sample order — the reference's value bit for bit at seed 12345."""
        sa, sb = stress_sample_pairs(self.graph, samples, seed)
        return self.stress_of_pairs(sa, sb)[0]

    def sort_quality(self):
        """gfs_ctx_sort_quality (1D contexts): dict(steps, abs_err_sum, genomic_sum, sq_err_sum) and the figures
        measure_layout_quality.rs derives from them (mse, rmse, mae, relative_error)."""
        q = SortQuality()
        check(lib().gfs_ctx_sort_quality(self._h, C.byref(q)))
        return sort_quality_figures(q.steps, q.abs_err_sum, q.genomic_sum, q.sq_err_sum)

    def path_errors(self, z=1, ratio=10.0, stream=None):
        """gfs_ctx_path_errors: per path, its steps, reverse steps, K7a's sums over its pairs (s, s + z) and how many of them
        are stretched (d_layout / d_path > ratio).  PATH_ERROR_DTYPE array, one row per path."""
        out = np.zeros(self.graph.n_paths, dtype=PATH_ERROR_DTYPE)
        check(lib().gfs_ctx_path_errors(self._h, C.c_uint64(z), C.c_double(ratio), _ptr(out), C.c_uint64(out.shape[0]),
                                        C.c_void_p(stream or 0)))
        return out

    def stretched_pairs(self, z=1, ratio=10.0, cap=1024, out=None, stream=None):
        """gfs_ctx_stretched_pairs: (the first min(cap, total) stretched pairs in ascending step_a as a STRETCHED_PAIR_DTYPE
        array, total).  out: a caller's array of at least cap entries to write into (entries beyond the list stay as they are)."""
        cap = int(cap)
        if out is None and cap:
            out = np.zeros(cap, dtype=STRETCHED_PAIR_DTYPE)
        if cap and (out.dtype != STRETCHED_PAIR_DTYPE or out.shape[0] < cap or not out.flags.c_contiguous):
            raise ValueError("out must be a contiguous STRETCHED_PAIR_DTYPE array of at least cap entries")
        total = C.c_uint64(0)
        check(lib().gfs_ctx_stretched_pairs(self._h, C.c_uint64(z), C.c_double(ratio), _ptr(out) if cap else None, C.c_uint64(cap),
                                            C.byref(total), C.c_void_p(stream or 0)))
        n = min(cap, int(total.value))
        return (out[:n] if cap else np.zeros(0, dtype=STRETCHED_PAIR_DTYPE)), int(total.value)

    def node_errors(self, z=1, ratio=10.0, stream=None):
        """gfs_ctx_node_errors: per dense node, the counted pairs (s, s + z) touching it, the stretched ones among them and the
        largest rel_sq.  NODE_ERROR_DTYPE array, one row per node."""
        out = np.zeros(self.graph.n_nodes, dtype=NODE_ERROR_DTYPE)
        check(lib().gfs_ctx_node_errors(self._h, C.c_uint64(z), C.c_double(ratio), _ptr(out), C.c_uint64(out.shape[0]),
                                        C.c_void_p(stream or 0)))
        return out

    # ---- test hooks ----
    def step_records(self):
        """The device step records, padding record included: uint32 array of shape (n_steps + 1, 4)."""
        out = np.zeros((self.graph.n_steps + 1, 4), dtype=np.uint32)
        check(lib().gfs_ctx_debug_step_records(self._h, _ptr(out), C.c_uint64(out.size)))
        return out

    def debug_sgd_state(self, which):
        """gfs_ctx_debug_sgd_state: state array `which` (STATE_*) of a set-up context as it lies on the device — float64 positions
        (device order) and zeta table, ITER_CONSTS_DTYPE schedule table, TERM_DTYPE trace, uint64 RNG words [k * n_streams + t] and
        counters, uint32 team state and trace counts; empty for an array the setup did not make."""
        dtype = {STATE_POSITIONS: np.float64, STATE_ZETAS: np.float64, STATE_SCHEDULE: ITER_CONSTS_DTYPE, STATE_TRACE: TERM_DTYPE,
                 STATE_RNG: np.uint64, STATE_COUNTERS: np.uint64, STATE_LEAD: np.uint32, STATE_TRACE_COUNTS: np.uint32}[int(which)]
        size = C.c_uint64(0)
        check(lib().gfs_ctx_debug_sgd_state(self._h, C.c_uint32(int(which) | STATE_SIZE_OF), C.byref(size), C.c_uint64(8)))
        out = np.zeros(int(size.value) // np.dtype(dtype).itemsize, dtype=dtype)
        check(lib().gfs_ctx_debug_sgd_state(self._h, C.c_uint32(int(which)), _ptr(out), C.c_uint64(out.nbytes)))
        return out

    def kshift(self, set=None):
        """Crowding onset the kernels are handed (needs a set-up context).  set: an int >= 0 overrides it for every
        later launch of this context, -1 restores the policy; None leaves it as it is."""
        v = C.c_int32(0)
        check(lib().gfs_ctx_debug_kshift(self._h, C.c_int32(-2 if set is None else int(set)), C.byref(v)))
        return int(v.value)

    def record_bytes(self):
        """Bytes of the per-step record the trips of the next launch read: 8 (trip records) or 16 (step records); 0 where the
        context is not set up or has no work."""
        return int(lib().gfs_ctx_record_bytes(self._h))

    def phase_window(self, set_begin=-1, set_end=-1):
        """GFS_F_PHASED's effective window (begin, end) of this context; set_begin, set_end >= 0 replace it for later launches
        (a test and probe hook)."""
        b, e = C.c_uint64(0), C.c_uint64(0)
        check(lib().gfs_ctx_phase_window(self._h, C.c_int64(int(set_begin)), C.c_int64(int(set_end)), C.byref(b), C.byref(e)))
        return int(b.value), int(e.value)


# ---- context sets: the contexts of many small graphs built in one pass ------------------------------
def ctx_set_plan(n_nodes, n_steps, n_paths):
    """gfs_ctx_set_plan (host only): (offsets as a uint64 array of shape (items, 5): step_rec, path_rec, path_len, perm, node_len;
    arena_bytes)."""
    nn, ns, npth = (np.ascontiguousarray(a, dtype=np.uint64) for a in (n_nodes, n_steps, n_paths))
    n = nn.shape[0]
    if ns.shape[0] != n or npth.shape[0] != n:
        raise ValueError("one count of each kind per item")
    off = np.zeros((max(n, 1), 5), dtype=np.uint64)
    total = C.c_uint64(0)
    check(lib().gfs_ctx_set_plan(_ptr(nn), _ptr(ns), _ptr(npth), C.c_uint64(n), _ptr(off), C.byref(total)))
    return off[:n], int(total.value)


def ctx_set_state_plan(nbytes):
    """gfs_ctx_set_state_plan (host only): nbytes[i][k] = bytes of item i's state array k (STATE_*).  Returns (offsets as a uint64
    array of shape (items, 8), arena_bytes)."""
    nb = np.ascontiguousarray(nbytes, dtype=np.uint64).reshape(-1, STATE_KINDS)
    off = np.zeros((max(nb.shape[0], 1), STATE_KINDS), dtype=np.uint64)
    total = C.c_uint64(0)
    check(lib().gfs_ctx_set_state_plan(_ptr(nb), C.c_uint64(nb.shape[0]), _ptr(off), C.byref(total)))
    return off[:nb.shape[0]], int(total.value)


class ContextSet:
    """gfs_ctx_set: one Context per graph, all built in one pass over the graphs' disjoint union (allocations, copies and
    launches do not grow with their number).  .contexts are ordinary Contexts — setup, runs, read-outs, hip.Batch — that do not
    destroy their handle: close() (or the set's collection) destroys them all, after any Batch made from them."""

    def __init__(self, graphs, device=0):
        self._h = C.c_void_p()
        self.contexts = []
        graphs = list(graphs)
        n = len(graphs)
        views, self._keep = [], []
        for g in graphs:
            v, keep = make_view(g)
            views.append(v)
            self._keep.append(keep)
        arr = (C.c_void_p * max(n, 1))(*[C.addressof(v) for v in views])
        check(lib().gfs_ctx_set_create(arr if n else None, C.c_uint64(n), C.c_int(device), C.byref(self._h)))
        self.contexts = [Context(g, _borrowed=lib().gfs_ctx_set_item(self._h, i)) for i, g in enumerate(graphs)]

    def close(self):
        if self._h:
            for c in self.contexts:
                c.close()
            lib().gfs_ctx_set_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = ContextSetInfo()
        check(lib().gfs_ctx_set_get_info(self._h, C.byref(out)))
        return out

    def _setup(self, entry, make, params, cfgs, dims_of):
        n = len(self.contexts)
        params = list(params) if isinstance(params, (list, tuple)) else [params] * n
        cfgs = list(cfgs) if isinstance(cfgs, (list, tuple)) else [cfgs] * n
        if len(params) != n or len(cfgs) != n:
            raise ValueError("params / cfgs: one for all items or one per item")
        made = [make(p) for p in params]
        c_params = (type(made[0]) * n)(*made)
        c_cfgs = None if all(c is None for c in cfgs) else (LaunchConfig * n)(*[c if c is not None else LaunchConfig() for c in cfgs])
        rcs = np.zeros(n, dtype=np.int32)
        check(entry(self._h, c_params, c_cfgs, _ptr(rcs)))
        for ctx, p, c in zip(self.contexts, params, cfgs):
            ctx.params, ctx.cfg, ctx.dims = p, c, dims_of(p)
        return rcs.tolist()

    def setup_1d(self, params, cfgs=None):
        """gfs_ctx_set_setup_1d: every item set up as Context.setup_1d would, in one pass.  params: one PathSGDParams for all items
        or a sequence of one per item; cfgs likewise (None: defaults).  Returns the per-item codes (OK or NOTHING_TO_DO)."""
        return self._setup(lib().gfs_ctx_set_setup_1d, make_sgd_params, params, cfgs, lambda p: 0)

    def setup_nd(self, params, cfgs=None):
        """gfs_ctx_set_setup_nd: the same for layouts (LayoutSGDParams; the items may differ in their dimensions)."""
        return self._setup(lib().gfs_ctx_set_setup_nd, make_layout_params, params, cfgs, lambda p: p.dimensions)

    @property
    def setup_info(self):
        """gfs_ctx_set_setup_info of the last set setup (zeros before the first)."""
        out = ContextSetSetupInfo()
        check(lib().gfs_ctx_set_get_setup_info(self._h, C.byref(out)))
        return out


# ---- batches: many configured contexts in one persistent launch -----------------------------------
def batch_plan(blocks, max_blocks):
    """gfs_batch_plan (host only): (launch_of_item as a list, n_launches) for items of `blocks` workgroups each, greedy in order."""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint64)
    launch_of = np.zeros(max(blocks.shape[0], 1), dtype=np.uint32)
    n = C.c_uint32(0)
    check(lib().gfs_batch_plan(_ptr(blocks), C.c_uint64(blocks.shape[0]), C.c_uint64(int(max_blocks)), _ptr(launch_of), C.byref(n)))
    return launch_of[:blocks.shape[0]].tolist(), int(n.value)


class Batch:
    """gfs_batch: set-up Contexts run together, every item's whole schedule in one launch (or as few as fit the device).  The
    contexts are borrowed: keep them alive and do not set them up again while the batch exists.  After run() each context is as
    if its own run() had been called (download(), sort_order(), the read-outs and stats() per item), except that the kernel time
    is the batch's."""

    def __init__(self, contexts, max_blocks_per_launch=0):
        self._h = C.c_void_p()
        self.contexts = list(contexts)
        n = len(self.contexts)
        arr = (C.c_void_p * max(n, 1))(*[c._h for c in self.contexts])
        cfg = BatchConfig(int(max_blocks_per_launch), (C.c_uint64 * 3)())
        check(lib().gfs_batch_create(arr if n else None, C.c_uint64(n), C.byref(cfg), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().gfs_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, stream=None):
        return check(lib().gfs_batch_run(self._h, C.c_void_p(stream or 0)))

    def stats(self):
        st = BatchStats()
        check(lib().gfs_batch_get_stats(self._h, C.byref(st)))
        return st

    def result_offsets(self):
        """offsets[i] = first node of item i in the packed arrays of results(); offsets[items] = their length."""
        off = np.zeros(len(self.contexts) + 1, dtype=np.uint64)
        check(lib().gfs_batch_result_offsets(self._h, _ptr(off), C.c_uint64(off.shape[0])))
        return off

    def init_positions(self, stream=None):
        """Context.init_positions() on every item, in one launch."""
        check(lib().gfs_batch_init_positions(self._h, C.c_void_p(stream or 0)))

    def results(self, positions=True, order=True, stream=None):
        """Every item's download() and sort_order() in one launch per padded segment length and two copies: (list of float64
        arrays, list of uint64 arrays, kernel_ms), one array per item in the order given; None for a list that was not asked for."""
        off = self.result_offsets()
        total = int(off[-1])
        x = np.zeros(total, dtype=np.float64) if positions else None
        o = np.zeros(total, dtype=np.uint32) if order else None
        ms = C.c_double(0.0)
        check(lib().gfs_batch_results(self._h, _ptr(x), _ptr(o), C.c_uint64(total), C.byref(ms), C.c_void_p(stream or 0)))
        cut = lambda a: [a[int(off[i]):int(off[i + 1])] for i in range(len(self.contexts))]
        return (cut(x) if positions else None, cut(o.astype(np.uint64)) if order else None, float(ms.value))

    def debug_sort_cap(self, cap):
        """Test hook: items of more than cap nodes take the per-item sort (0 restores SEGMENT_SORT_CAP)."""
        check(lib().gfs_batch_debug_sort_cap(self._h, C.c_uint64(int(cap))))

    # ---- a batch of layouts: every item's coordinates as one packed array (K4c / K6c) ----
    def coords_offsets(self):
        """offsets[i] = first double of item i in the packed coordinates (result_offsets() * 2 * D); offsets[items] = their length."""
        return self.result_offsets() * np.uint64(2 * self.contexts[0].dims)

    def upload_coords(self, coords, stream=None):
        """Context.upload() on every item in one copy and one launch.  coords: one float64 array per item (Layout.coords order,
        n_nodes * 2 * D each), or the packed array of all of them."""
        if isinstance(coords, (list, tuple)):
            coords = np.concatenate([np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in coords]) if coords else np.zeros(0)
        coords = np.ascontiguousarray(coords, dtype=np.float64).reshape(-1)
        buf = coords if coords.shape[0] else np.zeros(1)                 # (a pointer even where there is nothing to move)
        check(lib().gfs_batch_upload_coords(self._h, _ptr(buf), C.c_uint64(coords.shape[0]), C.c_void_p(stream or 0)))

    def coords(self, stream=None):
        """Every item's download() in one launch and one copy: (list of float64 views of one packed array, one per item in the
        order given; kernel_ms)."""
        if self.contexts[0].dims == 0:
            total, off = 0, None
        else:
            off = self.coords_offsets()
            total = int(off[-1])
        x = np.zeros(max(total, 1), dtype=np.float64)
        ms = C.c_double(0.0)
        check(lib().gfs_batch_coords(self._h, _ptr(x), C.c_uint64(total), C.byref(ms), C.c_void_p(stream or 0)))
        return [x[int(off[i]):int(off[i + 1])] for i in range(len(self.contexts))], float(ms.value)

    def pair_errors(self, zs, stream=None, return_ms=False):
        """Context.pair_errors(zs) of every item, sorts and layouts alike, in one step launch and one reduce launch: a
        PAIR_ERROR_DTYPE array of shape (items, len(zs)), row i bit for bit what contexts[i].pair_errors(zs) returns."""
        zs = np.ascontiguousarray(zs, dtype=np.uint64)
        out = np.zeros((len(self.contexts), zs.shape[0]), dtype=PAIR_ERROR_DTYPE)
        ms = C.c_double(0.0)
        check(lib().gfs_batch_pair_errors(self._h, _ptr(zs), C.c_uint64(zs.shape[0]), _ptr(out), C.byref(ms), C.c_void_p(stream or 0)))
        return (out, float(ms.value)) if return_ms else out

    # ---- the diagnosis of every item (K7h / K7i / K7j): one step distance and one ratio for the whole batch ----
    def path_offsets(self):
        """offsets[i] = first path of item i in the packed rows of path_errors(); offsets[items] = their number."""
        off = np.zeros(len(self.contexts) + 1, dtype=np.uint64)
        check(lib().gfs_batch_path_offsets(self._h, _ptr(off), C.c_uint64(off.shape[0])))
        return off

    def path_errors(self, z=1, ratio=10.0, stream=None, return_ms=False):
        """Context.path_errors(z, ratio) of every item in two launches: a list of per-item views of one packed PATH_ERROR_DTYPE
        array, item i's bit for bit what contexts[i].path_errors(z, ratio) returns."""
        off = self.path_offsets()
        out = np.zeros(int(off[-1]), dtype=PATH_ERROR_DTYPE)
        ms = C.c_double(0.0)
        check(lib().gfs_batch_path_errors(self._h, C.c_uint64(z), C.c_double(ratio), _ptr(out), C.c_uint64(out.shape[0]), C.byref(ms),
                                          C.c_void_p(stream or 0)))
        rows = [out[int(off[i]):int(off[i + 1])] for i in range(len(self.contexts))]
        return (rows, float(ms.value)) if return_ms else rows

    def stretched_pairs(self, z=1, ratio=10.0, cap=1024, out=None, stream=None, return_ms=False):
        """Context.stretched_pairs(z, ratio, cap) of every item in two launches and one scan: (list of rows[:min(cap, total_i)], a
        STRETCHED_PAIR_DTYPE array per item in ascending step_a, step and path numbers the item's own; totals as a uint64 array).
        out: a caller's (items, cap) array to write into (entries beyond an item's list stay as they are)."""
        cap, n = int(cap), len(self.contexts)
        if out is None:
            out = np.zeros((n, cap), dtype=STRETCHED_PAIR_DTYPE)
        if out.dtype != STRETCHED_PAIR_DTYPE or out.shape != (n, cap) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous STRETCHED_PAIR_DTYPE array of shape (items, cap)")
        totals = np.zeros(n, dtype=np.uint64)
        ms = C.c_double(0.0)
        check(lib().gfs_batch_stretched_pairs(self._h, C.c_uint64(z), C.c_double(ratio), _ptr(out) if cap else None, C.c_uint64(cap),
                                              _ptr(totals), C.byref(ms), C.c_void_p(stream or 0)))
        rows = [out[i, :min(cap, int(totals[i]))] for i in range(n)]
        return (rows, totals, float(ms.value)) if return_ms else (rows, totals)

    def node_errors(self, z=1, ratio=10.0, stream=None, return_ms=False):
        """Context.node_errors(z, ratio) of every item in two launches: a list of per-item views of one packed NODE_ERROR_DTYPE
        array, by dense node index, item i's at result_offsets()[i]."""
        off = self.result_offsets()
        out = np.zeros(int(off[-1]), dtype=NODE_ERROR_DTYPE)
        ms = C.c_double(0.0)
        check(lib().gfs_batch_node_errors(self._h, C.c_uint64(z), C.c_double(ratio), _ptr(out), C.c_uint64(out.shape[0]), C.byref(ms),
                                          C.c_void_p(stream or 0)))
        rows = [out[int(off[i]):int(off[i + 1])] for i in range(len(self.contexts))]
        return (rows, float(ms.value)) if return_ms else rows

    def sort_quality(self, stream=None, return_kernel_ms=False):
        """Context.sort_quality() of every item of a batch of 1D sorts, in one launch per padded segment length, one step launch
        and one reduce launch: a list of dicts, item i's field for field what contexts[i].sort_quality() returns."""
        n = len(self.contexts)
        out = np.zeros(n, dtype=SORT_QUALITY_DTYPE)
        ms = C.c_double(0.0)
        check(lib().gfs_batch_sort_quality(self._h, _ptr(out), C.c_uint64(n), C.byref(ms), C.c_void_p(stream or 0)))
        rows = [sort_quality_figures(r["steps"], r["abs_err_sum"], r["genomic_sum"], float(r["sq_err_sum"])) for r in out]
        return (rows, float(ms.value)) if return_kernel_ms else rows

    def debug_tile_blocks(self, n):
        """Test hook: at most n workgroups in the grids over tiles and paths of path_errors() and stretched_pairs() (0 restores the
        default).  No result depends on it."""
        check(lib().gfs_batch_debug_tile_blocks(self._h, C.c_uint64(int(n))))


# ---- one-shot entry points ---------------------------------------------------------------------
def path_linear_sgd_raw(g, p, x=None, cfg=None, etas=None, zetas=None):
    """gfs_path_linear_sgd.  Returns (rc, x, stats)."""
    v, keep = make_view(g)
    sp = make_sgd_params(p)
    init = 1 if x is None else 0
    if x is None:
        x = np.zeros(g.n_nodes, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    st = Stats()
    rc = check(lib().gfs_path_linear_sgd(C.byref(v), C.byref(sp), C.byref(cfg) if cfg is not None else None,
                                         _ptr(etas), _ptr(zetas), C.c_int(init), _ptr(x), C.byref(st)))
    return rc, x, st


def path_sgd_sort_raw(g, p, x=None, cfg=None, etas=None, zetas=None):
    """gfs_path_sgd_sort.  Returns (rc, x, order, stats)."""
    v, keep = make_view(g)
    sp = make_sgd_params(p)
    init = 1 if x is None else 0
    if x is None:
        x = np.zeros(g.n_nodes, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    order = np.zeros(g.n_nodes, dtype=np.uint64)
    st = Stats()
    rc = check(lib().gfs_path_sgd_sort(C.byref(v), C.byref(sp), C.byref(cfg) if cfg is not None else None,
                                       _ptr(etas), _ptr(zetas), C.c_int(init), _ptr(x), _ptr(order), C.byref(st)))
    return rc, x, order, st


def path_linear_sgd_layout_raw(g, p, coords, cfg=None, etas=None, zetas=None):
    """gfs_path_linear_sgd_layout.  coords: float64[n_nodes*2*D] Layout order, updated copy returned."""
    v, keep = make_view(g)
    lp = make_layout_params(p)
    coords = np.ascontiguousarray(coords, dtype=np.float64).copy()
    st = Stats()
    rc = check(lib().gfs_path_linear_sgd_layout(C.byref(v), C.byref(lp), C.byref(cfg) if cfg is not None else None,
                                                _ptr(etas), _ptr(zetas), _ptr(coords), C.byref(st)))
    return rc, coords, st
