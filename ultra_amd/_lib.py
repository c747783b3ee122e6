"""ctypes binding of libultra_amd.so (include/ultra_rspmm.h).

PyTorch only supplies device memory (tensor.data_ptr()) and the current HIP stream; every kernel is
ours.  There is NO fallback: if the shared library is missing or fails to load, importing this
module raises, and CPU tensors are rejected by the callers.
"""
import ctypes
import os

# PyTorch-ROCm ships its own HIP runtime; it must be the one already resident when libultra_amd.so resolves
# libamdhip64 (a second runtime in the process sees "no ROCm-capable device").  Hence torch first.
import torch  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
# ULTRA_AMD_LIB: another build of the same sources (kernel A/B measurements, tools/build_variant.py)
LIB_PATH = os.environ.get("ULTRA_AMD_LIB") or os.path.join(HERE, "lib", "libultra_amd.so")

ULTRA_OK = 0
ULTRA_ERR_INVALID = 1
ULTRA_ERR_UNSORTED = 2
ULTRA_ERR_HIP = 3
ULTRA_ERR_UNSUPPORTED = 4

SUM_CODES = {"add": 0, "min": 1, "max": 2}
MUL_CODES = {"mul": 0, "add": 1, "rotate": 2}      # rotate: ULTRA_MUL_ROTATE (the plan API only)
F32, F64 = 0, 1

ARR_ROW_PTR, ARR_COL, ARR_TYPE, ARR_PERM, ARR_ITEM, ARR_SPLIT_ROW, ARR_SPLIT_PTR = range(7)
PLAN_EXACT_ORDER = 1
PLAN_TYPE_RUNS = 2
PLAN_DENSE = 4
LAYER_REFERENCE_ORDER = 8
DENSE_MAX_IN_ROW = 1024
BEAM_MAX = 64                # ULTRA_BEAM_MAX
BEAM_HUB_DEGREE = 256        # ULTRA_BEAM_HUB_DEGREE
RANKING_LDS_ANSWERS = 2048   # ULTRA_RANKING_LDS_ANSWERS
TOPK_MAX = 256               # ULTRA_TOPK_MAX
TOPK_CHUNK = 4096            # ULTRA_TOPK_CHUNK
ABOVE_MAX_BATCH = 65535      # the most rows ultra_filtered_above takes
PAIRS_MAX_BATCH = 65535      # the most rows ultra_topk_pairs_merge takes (csrc/pairs_kernels.hip PAIRS_MAX_BATCH)
ARR_DENSE = 7
ARR_DENSE_ORDER = 8
# the layer update's flag bits: ULTRA_CONV_* and, for ultra_nbf_layer0 alone, ULTRA_LAYER0_* (include/ultra_nbfnet.h)
CONV_LAYER_NORM, CONV_RELU, CONV_RESIDUAL = 1, 2, 4
LAYER0_MAX, LAYER0_ONLY_FILL, LAYER0_SKIP_FILL = 8, 16, 32
# the bits of ultra_relation_graph_add_edges' `changed` word
RELGRAPH_CHANGED, RELGRAPH_OUT_OF_RANGE = 1, 2


class UltraMat(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("n_outer", ctypes.c_int64), ("stride_outer", ctypes.c_int64),
                ("n_row", ctypes.c_int64), ("stride_row", ctypes.c_int64), ("row_len", ctypes.c_int64)]


class UltraDelta(ctypes.Structure):
    """ultra_delta: the device arrays of a graph delta (include/ultra_rspmm.h, ultra_rspmm_delta_rows)."""
    _fields_ = [("row_dev", ctypes.c_void_p), ("ptr_dev", ctypes.c_void_p), ("col_dev", ctypes.c_void_p),
                ("type_dev", ctypes.c_void_p), ("count_dev", ctypes.c_void_p), ("capacity_rows", ctypes.c_int64),
                ("capacity_edges", ctypes.c_int64)]


class UltraTombstones(ctypes.Structure):
    """ultra_tombstones: the dead (col, type) keys of a graph delta's touched rows (ultra_rspmm_edit_rows)."""
    _fields_ = [("ptr_dev", ctypes.c_void_p), ("col_dev", ctypes.c_void_p), ("type_dev", ctypes.c_void_p),
                ("capacity_keys", ctypes.c_int64)]


class UltraSampleKeys(ctypes.Structure):
    """ultra_sample_keys: per outer slice the (row, col, type) keys of the edges that slice must not see
    (ultra_rspmm_edit_rows_samples)."""
    _fields_ = [("row_dev", ctypes.c_void_p), ("col_dev", ctypes.c_void_p), ("type_dev", ctypes.c_void_p),
                ("per_sample", ctypes.c_int64)]


class UltraExplainEdits(ctypes.Structure):
    """ultra_explain_edits: a graph delta keyed by destination, with the transpose of its added edges, for the explanation
    route (include/ultra_rspmm.h, ultra_rspmm_delta_edges_forward; ultra_beam_search_edit_rows_batch)."""
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "row_dev", "count_dev", "add_ptr_dev", "add_src_dev", "add_dst_dev", "add_type_dev", "add_j_dev", "dead_ptr_dev",
        "dead_src_dev", "dead_type_dev", "src_row_dev", "src_count_dev", "src_ptr_dev", "src_dst_dev", "src_type_dev")] + [
        ("capacity_rows", ctypes.c_int64), ("capacity_edges", ctypes.c_int64), ("capacity_keys", ctypes.c_int64)]


class UltraTraversalEdits(ctypes.Structure):
    """ultra_traversal_edits: a graph delta in the symbolic traversal's direction (include/ultra_nbfnet.h,
    ultra_symbolic_traversal_edit_rows)."""
    _fields_ = [("row_dev", ctypes.c_void_p), ("count_dev", ctypes.c_void_p), ("add_ptr_dev", ctypes.c_void_p),
                ("add_src_dev", ctypes.c_void_p), ("add_type_dev", ctypes.c_void_p), ("dead_ptr_dev", ctypes.c_void_p),
                ("dead_src_dev", ctypes.c_void_p), ("dead_type_dev", ctypes.c_void_p), ("capacity_rows", ctypes.c_int64),
                ("capacity_edges", ctypes.c_int64), ("capacity_keys", ctypes.c_int64)]


class PlanOpts(ctypes.Structure):
    _fields_ = [("seg_len", ctypes.c_int32), ("g_max", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class PlanInfo(ctypes.Structure):
    _fields_ = [("num_edge", ctypes.c_int64), ("num_node", ctypes.c_int64), ("num_relation", ctypes.c_int64),
                ("n_item", ctypes.c_int64), ("n_wave_item", ctypes.c_int64), ("n_group_item", ctypes.c_int64),
                ("n_unit", ctypes.c_int64), ("n_split_row", ctypes.c_int64), ("n_partial_slot", ctypes.c_int64),
                ("seg_len", ctypes.c_int32), ("g_max", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("packed", ctypes.c_int32), ("on_device", ctypes.c_int32), ("has_transpose", ctypes.c_int32),
                ("n_type_run", ctypes.c_int64), ("dense_bytes", ctypes.c_int64), ("n_chain_row", ctypes.c_int64),
                ("dense_order_bytes", ctypes.c_int64)]


class ScheduleInfo(ctypes.Structure):
    _fields_ = [("nparts", ctypes.c_int32), ("reserved", ctypes.c_int32), ("n_chunk", ctypes.c_int64),
                ("n_unit", ctypes.c_int64), ("max_chunk_per_part", ctypes.c_int64), ("max_unit_per_part", ctypes.c_int64),
                ("max_cost", ctypes.c_double), ("mean_cost", ctypes.c_double)]


class Tuning(ctypes.Structure):
    _fields_ = [("threads", ctypes.c_int32), ("grid", ctypes.c_int32), ("rel_lds", ctypes.c_int32),
                ("x_lds", ctypes.c_int32), ("unroll", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "ultra_amd: %s is missing. Build it with `python -m ultra_amd.build` (needs hipcc); "
            "there is no CPU or PyTorch fallback for the rspmm engine." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    lib.ultra_last_error.restype = ctypes.c_char_p
    lib.ultra_abi_version.restype = ctypes.c_int32
    lib.ultra_device_count.restype = ctypes.c_int32
    lib.ultra_device_error.restype = ctypes.c_int32
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    matp = ctypes.POINTER(UltraMat)
    lib.ultra_plan_create.argtypes = [ctypes.POINTER(vp), vp, vp, i64, i64, i64, i64, ctypes.POINTER(PlanOpts)]
    lib.ultra_plan_upload.argtypes = [vp]
    lib.ultra_plan_destroy.argtypes = [vp]
    lib.ultra_plan_pin.argtypes = [vp, i32]
    lib.ultra_plan_get_info.argtypes = [vp, ctypes.POINTER(PlanInfo)]
    lib.ultra_plan_export.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64)]
    lib.ultra_rspmm_forward.argtypes = [vp, i32, i32, i32, vp, matp, matp, matp, matp, vp]
    lib.ultra_rspmm_forward_masked.argtypes = [vp, i32, i32, i32, vp, matp, matp, matp, matp, vp]
    lib.ultra_rspmm_forward_masked_samples.argtypes = [vp, i32, i32, i32, vp, i64, matp, matp, matp, matp, vp]
    lib.ultra_rspmm_delta_rows.argtypes = [vp, i32, i32, i32, matp, matp, matp, vp, matp, ctypes.POINTER(UltraDelta), vp]
    lib.ultra_rspmm_edit_rows.argtypes = [vp, i32, i32, i32, matp, matp, matp, vp, matp, ctypes.POINTER(UltraDelta),
                                          ctypes.POINTER(UltraTombstones), vp]
    lib.ultra_rspmm_edit_rows_samples.argtypes = [vp, i32, i32, i32, matp, matp, matp, vp, matp, ctypes.POINTER(UltraDelta),
                                                  ctypes.POINTER(UltraTombstones), ctypes.POINTER(UltraSampleKeys), vp]
    lib.ultra_rspmm_edit_rows_split.argtypes = [vp, i32, i32, i32, matp, matp, matp, vp, matp, ctypes.POINTER(UltraDelta),
                                                ctypes.POINTER(UltraTombstones), ctypes.POINTER(UltraSampleKeys), i64, vp]
    lib.ultra_rspmm_edit_rows_owned.argtypes = [vp, i32, i32, i32, matp, matp, matp, vp, matp, ctypes.POINTER(UltraDelta), vp,
                                                ctypes.POINTER(UltraTombstones), i64, vp]
    lib.ultra_rspmm_hub_tile.restype = i32
    lib.ultra_rspmm_forward_onehot.argtypes = [vp, i32, vp, matp, matp, vp, matp, matp, vp]
    lib.ultra_rspmm_forward_point.argtypes = [vp, i32, i32, i32, vp, matp, matp, vp, matp, matp, vp]
    lib.ultra_rspmm_forward_update.argtypes = [vp, i32, i32, matp, matp, vp, matp, matp, vp, vp, vp, vp, ctypes.c_float, i32, matp, vp]
    lib.ultra_rspmm_forward_update_timed.argtypes = [vp, i32, i32, matp, matp, vp, matp, matp, vp, vp, vp, vp, ctypes.c_float, i32, matp, vp,
                                                     i32, i32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    lib.ultra_nbf_dense_layer.argtypes = [vp, matp, matp, matp, vp, vp, vp, vp, vp, ctypes.c_float, i32, matp, vp]
    lib.ultra_nbf_layer0.argtypes = [vp, vp, matp, vp, vp, vp, vp, vp, vp, ctypes.c_float, i32, matp, vp]
    # the two on a byte adjacency that is an operand: (a_ex, num_node) in place of the plan
    lib.ultra_nbf_dense_layer_adjacency.argtypes = [vp, i64, matp, matp, matp, vp, vp, vp, vp, vp, ctypes.c_float, i32, matp, vp]
    lib.ultra_nbf_dense_layer0_adjacency.argtypes = [vp, i64, matp, vp, vp, vp, vp, vp, vp, ctypes.c_float, i32, matp, vp]
    lib.ultra_rspmm_backward.argtypes = [vp, i32, i32, i32, vp, matp, matp, matp, matp, vp, matp, matp, vp]
    lib.ultra_rspmm_backward_add.argtypes = [vp, i32, i32, i32, vp, matp, matp, matp, matp, vp, matp, matp, matp, vp]
    lib.ultra_rspmm_edge_grad_samples.argtypes = [vp, i32, i32, i32, matp, matp, matp, vp, i64, vp]
    lib.ultra_rspmm_dense_relation_grad.argtypes = [vp, matp, matp, matp, vp]
    lib.ultra_rspmm_rows_forward.argtypes = [vp, i32, vp, matp, matp, vp, i64, matp, vp, vp, vp, vp]
    lib.ultra_rspmm_rows_backward.argtypes = [vp, i32, vp, matp, matp, vp, i64, vp, matp, matp, vp]
    lib.ultra_rspmm_rows_backward_gather.argtypes = [vp, i32, vp, matp, matp, vp, i64, vp, vp, vp, vp, matp, matp, vp]
    lib.ultra_rspmm_weight_epoch.argtypes = [i64]
    lib.ultra_rspmm_onehot_backward.argtypes = [vp, vp, vp, vp, vp, matp, vp, vp, matp, vp, vp, vp]
    lib.ultra_rspmm_forward_timed.argtypes = [vp, i32, i32, i32, vp, matp, matp, matp, vp, matp, vp, i32, i32,
                                              ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    lib.ultra_conv_update.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, ctypes.c_float, i32, vp]
    lib.ultra_conv_update_backward_workspace.argtypes = [i64]
    lib.ultra_conv_update_backward_workspace.restype = i64
    lib.ultra_conv_update_backward.argtypes = [vp] * 14 + [i64, i64, i32, i32, ctypes.c_float, i32, vp]
    lib.ultra_edge_keep_mask.argtypes = [vp, vp, vp, i64, vp, i64, i64, i64, vp, vp]
    lib.ultra_easy_edge_keep.argtypes = [vp, vp, vp, i64, vp, vp, vp, i64, i64, i64, i64, i64, vp, vp]
    lib.ultra_leave_one_out_keep.argtypes = [vp, vp, vp, i64, vp, vp, vp, i64, i64, i64, i64, i64, vp, i64, vp]
    lib.ultra_easy_edge_keep_table_workspace.argtypes = [i64]
    lib.ultra_easy_edge_keep_table_workspace.restype = i64
    lib.ultra_easy_edge_keep_table.argtypes = [vp, vp, vp, i64, vp, vp, vp, i64, i64, i64, i64, i64, vp, i64, vp, vp]
    lib.ultra_readout.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, i32, i32, vp]
    lib.ultra_stream_copy.argtypes = [vp, vp, i64, vp]
    lib.ultra_filtered_rank.argtypes = [vp, vp, vp, vp, i64, i64, vp, vp, vp]
    lib.ultra_filtered_topk_workspace.argtypes = [i64, i64, i32]
    lib.ultra_filtered_topk_workspace.restype = i64
    lib.ultra_filtered_topk.argtypes = [vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, i64, vp]
    # the live-count twins: the parent's arguments plus a device pointer to the int64 live count before the stream
    lib.ultra_filtered_rank_live.argtypes = [vp, vp, vp, vp, i64, i64, vp, vp, vp, vp]
    lib.ultra_filtered_topk_live.argtypes = [vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, i64, vp, vp]
    lib.ultra_filtered_above_live.argtypes = [vp, vp, vp, i64, i64, ctypes.c_float, vp, vp, vp, i64, vp, vp, i64, vp, vp]
    # the twins over the ids that are alive: the _live arguments plus the retired bitmap and the device pointer to
    # the int64 retired count, before the stream
    lib.ultra_filtered_rank_alive.argtypes = [vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp, vp]
    lib.ultra_filtered_topk_alive.argtypes = [vp, vp, vp, i64, i64, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    lib.ultra_filtered_above_alive.argtypes = [vp, vp, vp, i64, i64, ctypes.c_float, vp, vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]
    lib.ultra_filtered_above_workspace.argtypes = [i64, i64]
    lib.ultra_filtered_above_workspace.restype = i64
    lib.ultra_filtered_above.argtypes = [vp, vp, vp, i64, i64, ctypes.c_float, vp, vp, vp, i64, vp, vp, i64, vp]
    # the selections among a candidate list per row: the parent's arguments with (among_span, among_index) behind
    # the known lists and among_capacity behind n_cand; the live count, the retired bitmap and the retired count (None each:
    # absent) before the stream
    lib.ultra_filtered_topk_among_workspace.argtypes = [i64, i64, i32]
    lib.ultra_filtered_topk_among_workspace.restype = i64
    lib.ultra_filtered_topk_among.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    lib.ultra_filtered_above_among_workspace.argtypes = [i64, i64]
    lib.ultra_filtered_above_among_workspace.restype = i64
    lib.ultra_filtered_above_among.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, ctypes.c_float, vp, vp, vp, i64, vp, vp, i64,
                                               vp, vp, vp, vp]
    lib.ultra_filtered_rank_among.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    # the best k (query, id, score) records over many queries: (ids, scores, batch, k_row, query_base, n_rows or
    # None, min_score or None, best_query, best_id, best_score, best_count, k, stream)
    lib.ultra_topk_pairs_merge.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.ultra_query_segment.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, i32, vp, vp, i64, vp, i64, vp, vp, vp, vp]
    lib.ultra_nonzero_lists.argtypes = [vp, i64, i64, vp, vp, vp, i64, vp]
    # ... over the live ids of rows of n slots: the device pointer to the int64 live count before the stream
    lib.ultra_nonzero_lists_live.argtypes = [vp, i64, i64, vp, vp, vp, i64, vp, vp]
    # ... without the retired ids: the live count (or None: every slot) and the retired bitmap before the stream
    lib.ultra_nonzero_lists_alive.argtypes = [vp, i64, i64, vp, vp, vp, i64, vp, vp, vp]
    lib.ultra_beam_search_layer.argtypes =[vp, vp, vp, vp, vp, i64, i64, i64, vp, vp, i64, i32, vp, vp, vp]
    lib.ultra_beam_search_layer_batch.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, i32, vp, vp, vp]
    editsp = ctypes.POINTER(UltraExplainEdits)
    lib.ultra_beam_search_edit_rows_batch.argtypes = [vp, vp, vp, vp, i64, i64, i64, vp, editsp, vp, i64, vp, vp, i32, vp, vp, vp]
    lib.ultra_rspmm_delta_edges_forward.argtypes = [editsp, matp, matp, matp, vp]
    lib.ultra_rspmm_delta_edges_backward_input.argtypes = [editsp, matp, matp, matp, vp]
    lib.ultra_rspmm_delta_edge_grad_samples.argtypes = [editsp, matp, matp, matp, vp, i64, vp]
    lib.ultra_symbolic_traversal.argtypes = [vp, vp, vp, i64, vp, i64, i32, vp, vp, vp]
    lib.ultra_symbolic_traversal_edit_rows.argtypes = [vp, vp, vp, i64, ctypes.POINTER(UltraTraversalEdits), vp, i64, i32, vp,
                                                       vp, vp]
    lib.ultra_symbolic_traversal_edit_rows_owned.argtypes = [vp, vp, vp, i64, ctypes.POINTER(UltraTraversalEdits), vp, vp, i64, i32,
                                                             vp, vp, vp]
    lib.ultra_answer_ranking.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, vp, vp]
    lib.ultra_strict_negatives.argtypes = [vp, i64, vp, vp, vp, vp, i64, i64, i64, i64, vp, vp]
    lib.ultra_ranking_loss.argtypes = [vp, i64, i64, ctypes.c_float, ctypes.c_float, vp, vp, vp]
    lib.ultra_readout_train_forward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp]
    lib.ultra_readout_train_backward_workspace.argtypes = [i64, i64]
    lib.ultra_readout_train_backward_workspace.restype = i64
    lib.ultra_readout_train_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, vp]
    lib.ultra_onehot_rows.argtypes = [vp, vp, vp, i64, i64, i64, vp]
    lib.ultra_batch_prologue.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    lib.ultra_batch_prologue_rows.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.ultra_readout_batch.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64, i64, i32, i32, vp]
    lib.ultra_query_boundary.argtypes = [vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp]
    lib.ultra_relation_projection.argtypes = [vp, vp, vp, vp, vp, vp, i64, i32, i32, vp]
    pp = ctypes.POINTER(vp)
    lib.ultra_relation_projection_layers.argtypes = [vp, pp, pp, pp, pp, vp, i64, i32, i32, vp]
    lib.ultra_relation_projection_backward_workspace.argtypes = [i64, i32]
    lib.ultra_relation_projection_backward_workspace.restype = i64
    lib.ultra_relation_projection_backward.argtypes = [vp, pp, pp, pp, pp, vp, vp, vp, vp, vp, vp, i64, i64, i32, i32, vp]
    lib.ultra_plan_schedule_info.argtypes = [vp, i32, ctypes.POINTER(ScheduleInfo)]
    lib.ultra_order_trace.argtypes = [vp]
    lib.ultra_plan_schedule_export.argtypes = [vp, i32, i32, vp, i64, ctypes.POINTER(i64)]
    lib.ultra_relation_graph_bits.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, vp, vp]
    lib.ultra_relation_graph_emit.argtypes = [vp, vp, i64, i64, vp, vp, vp]
    lib.ultra_relation_graph_dense_adjacency.argtypes = [vp, i64, vp, vp]
    lib.ultra_relation_graph_bits_keep.argtypes = [vp, vp, vp, i64, i64, i64, vp, vp, vp, vp, vp]
    lib.ultra_relation_graph_edge_keep.argtypes = [vp, i64, vp, vp, i64, vp, vp]
    lib.ultra_relation_graph_add_edges.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, vp]
    lib.ultra_symbolic_traversal_keep.argtypes = [vp, vp, vp, vp, i64, vp, i64, i32, vp, vp, vp]
    lib.ultra_traversal_dropout_mask_words.argtypes = [i64]
    lib.ultra_traversal_dropout_mask_words.restype = i64
    lib.ultra_traversal_dropout.argtypes = [vp, vp, i64, i64, i64, i32, vp, vp, vp, i64, i32, vp, vp, vp, vp, ctypes.c_float,
                                            vp, vp, vp, vp]
    lib.ultra_query_loss.argtypes = [vp, vp, i64, i64, ctypes.c_float, vp, vp, vp, vp]
    lib.ultra_set_tuning.argtypes = [ctypes.POINTER(Tuning)]
    lib.ultra_get_tuning.argtypes = [ctypes.POINTER(Tuning)]
    for s in ("add", "min", "max"):
        for m in ("mul", "add"):
            f = getattr(lib, "ultra_rspmm_%s_%s_forward_cuda" % (s, m))
            f.argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i32, vp]
            b = getattr(lib, "ultra_rspmm_%s_%s_backward_cuda" % (s, m))
            b.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i32, vp]
    return lib


lib = _load()
if lib.ultra_abi_version() != 7:
    raise ImportError("ultra_amd: libultra_amd.so ABI version mismatch")
# base slots per tile of the hub-row walker (ultra_rspmm_edit_rows_split; csrc/delta_kernels.hip HUB_TILE)
HUB_TILE = int(lib.ultra_rspmm_hub_tile())


class UltraError(RuntimeError):
    pass


def check(rc):
    """Map ultra_status to the exceptions the reference raises for the same condition."""
    if rc == ULTRA_OK:
        return
    msg = lib.ultra_last_error().decode("utf-8", "replace")
    if rc == ULTRA_ERR_UNSORTED:
        raise AssertionError(msg)           # rspmm.py:18
    raise UltraError(msg)                    # c10::Error -> RuntimeError in the reference


def stream_of(x):
    """The current HIP stream of a tensor's device, or of a device (the C entry points make that device current for the launch)."""
    return ctypes.c_void_p(torch.cuda.current_stream(x.device if isinstance(x, torch.Tensor) else x).cuda_stream)


def ptr(t):
    return t.data_ptr() if t is not None else None


def update_args(linear, layer_norm, relu, residual=False, extra_flags=0):
    """(weight, bias, ln_weight, ln_bias, eps, flags) of the layer update `[x +] relu(layer_norm(linear(cat[x, agg])))` as
    the entry points take it: None for an absent tensor, the default eps where there is no LayerNorm."""
    ln = layer_norm
    flags = (CONV_LAYER_NORM if ln is not None else 0) | (CONV_RELU if relu else 0) | (CONV_RESIDUAL if residual else 0) \
        | extra_flags
    return (linear.weight, linear.bias, ln.weight if ln is not None else None, ln.bias if ln is not None else None,
            float(ln.eps) if ln is not None else 1e-5, flags)
