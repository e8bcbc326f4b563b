"""ctypes binding of libgripnet_hip.so (the C ABI declared in include/gripnet_hip.h).

Nothing here depends on libtorch's ABI: tensors cross the boundary as raw device pointers,
sizes, leading dimensions and the current HIP stream.  There is no CPU fallback: if the
library is missing or a tensor is not on the GPU the call raises.
"""
from __future__ import annotations

import ctypes as C
import operator
import os
import threading

import torch

from ._cache import MISS, VersionedCache

# GN_HIP_LIBRARY selects another build of the same library (the diagnostic `make STAMPS=1` one)
_LIB_PATH = os.environ.get("GN_HIP_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                            "libgripnet_hip.so")
_lib = None
_lock = threading.Lock()

GN_OK, GN_ERR_INVALID_ARG, GN_ERR_HIP, GN_ERR_INDEX_RANGE, GN_ERR_UNSUPPORTED, GN_ERR_EDGE_COUNT = range(6)
GN_RGCN_PARTIAL, GN_RGCN_ARITH_FAST, GN_RGCN_BASIS_TRANSPOSED, GN_RGCN_SUM = 1, 4, 64, 128   # flags of gn_rgcn_forward_f32
GN_RGCN_PATH_SHIFT = 8
RGCN_PATHS = {"auto": 0, "pair": 1, "lds": 3, "general": 4, "table": 5}                  # kernel choice (tests, measurements)
RGCN_PATH_NAMES = {code: name for name, code in RGCN_PATHS.items()}
GN_GEMM_RELU, GN_GEMM_ARITH_FAST, GN_GEMM_B_TRANSPOSED, GN_GEMM_ACCUMULATE, GN_GEMM_A_TRANSPOSED, GN_GEMM_JOIN_BATCH, GN_GEMM_OUT_BF16 = 1, 2, 4, 8, 16, 32, 64                                    # flags of gn_gemm_f32
GN_DM_TYPES_SORTED = 1                                 # flags of gn_distmult_backward_ex_f32
GN_DM_TYPE_TASKS = 2
ABI_VERSION = 173                                       # GN_VERSION of include/gripnet_hip.h this module binds

_p, _i64, _int, _sz = C.c_void_p, C.c_int64, C.c_int, C.c_size_t

# name -> (restype, argtypes); mirrors include/gripnet_hip.h one to one
SIGNATURES = {
    "gn_version": (_int, []),
    "gn_last_error": (C.c_char_p, []),
    "gn_time_next_launch": (_int, [_p, _p]),
    "gn_host_scratch_release": (_sz, []),
    "gn_device_blocks_live": (_i64, []),
    "gn_time_launch_pending": (_int, []),
    "gn_gcn_plan_create": (_int, [_p, _p, _p, _i64, _i64, _int, _p, C.POINTER(_p)]),
    "gn_bipartite_plan_create": (_int, [_p, _p, _p, _i64, _i64, _i64, _p, C.POINTER(_p)]),
    "gn_sum_plan_create": (_int, [_p, _p, _p, _i64, _i64, _i64, _p, C.POINTER(_p)]),
    "gn_graph_plan_destroy": (None, [_p]),
    "gn_graph_plan_input_edges": (_i64, [_p]),
    "gn_graph_plan_nnz": (_i64, [_p]),
    "gn_graph_plan_export": (_int, [_p, _p, _p, _p]),
    "gn_graph_aggregate_f32": (_int, [_p, _p, _i64, _i64, _p, _i64, _p, _int, _p, _i64, _p, _p, _p]),
    "gn_split_planes_bytes": (_sz, [_i64, _int]),
    "gn_split_planes_f32": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p]),
    "gn_transform_fusable": (_int, [_i64, _i64]),
    "gn_graph_transform_fusable": (_int, [_p, _i64, _i64]),
    "gn_graph_plan_build_blocked": (_int, [_p, _i64, _p]),
    "gn_graph_plan_blocked_cols": (_i64, [_p]),
    "gn_graph_plan_blocked_gather_kernel": (_int, [_p]),
    "gn_graph_plan_blocked_waves": (_i64, [_p, _p, _i64]),
    "gn_graph_blocked_applicable": (_int, [_p, _p, _i64, _i64, _p, _i64, _p, _p, _i64]),
    "gn_graph_chain_applicable": (_int, [_p, _p, _p, _i64, _i64, _p, _i64, _p, _p, _i64, _p]),
    "gn_graph_aggregate_chain_f32": (_int, [_p, _p, _p, _i64, _i64, _p, _i64, _p, _int, _p, _i64, _p, _p]),
    "gn_graph_gather_chained_f32": (_int, [_p, _p, _i64, _p]),
    "gn_graph_aggregate_tail_f32": (_int, [_p, _p, _i64, _i64, _p, _i64, _p, _int, _p, _i64, _p, _p, _p, _p, _int, _p]),
    "gn_graph_split_applicable": (_int, [_p, _p, _i64, _i64, _p, _i64, _i64, _i64]),
    "gn_graph_aggregate_split_f32": (_int, [_p, _p, _i64, _i64, _p, _i64, _i64, _p, _i64, _p, _int, _p, _i64, _p, _p, _p]),
    "gn_graph_plan_build_transpose": (_int, [_p, _p]),
    "gn_graph_aggregate_t_f32": (_int, [_p, _p, _i64, _i64, _p, _i64, _p]),
    "gn_xtg_wide_supported": (_int, [_i64, _i64, _i64]),
    "gn_gemm_f32": (_int, [_p, _i64, _i64, _p, _i64, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _int, _p]),
    "gn_gemm_addend_f32": (_int, [_p, _i64, _i64, _p, _i64, _p, _i64, _i64, _p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p, _i64, _int, _p]),
    "gn_merge_f32": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _int, _p]),
    "gn_softmax_rows_f32": (_int, [_p, _i64, _i64, _i64, _p]),
    "gn_softmax_rows_backward_f32": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _i64, _p]),
    "gn_class_scores_f32": (_int, [_p, _i64, _i64, _p, _i64, _p, _i64, _i64, _i64, _int, _p, _i64, _p]),
    "gn_rgcn_plan_create": (_int, [_p, _p, _p, _int, _i64, _i64, _i64, _i64, _i64, _p, C.POINTER(_p)]),
    "gn_rgcn_plan_create_ex": (_int, [_p, _p, _p, _int, _i64, _i64, _i64, _i64, _i64, _int, _p, C.POINTER(_p)]),
    "gn_rgcn_plan_destroy": (None, [_p]),
    "gn_rgcn_plan_input_edges": (_i64, [_p]),
    "gn_rgcn_workspace_bytes": (_sz, [_p, _i64, _i64, _i64, _int]),
    "gn_rgcn_forward_path": (_int, [_p, _i64, _i64, _i64, _int]),
    "gn_rgcn_forward_choice": (_int, [_p, _p, _i64, _i64, _i64, _i64, _int, C.POINTER(_sz)]),
    "gn_cast_bf16": (_int, [_p, _i64, _p, _i64, _i64, _i64, _p]),
    "gn_graph_aggregate_bf16": (_int, [_p, _p, _i64, _i64, _p, _int, _p, _i64, _p, _p]),
    "gn_rgcn_forward_f32": (_int, [_p, _p, _i64, _i64, _p, _p, _i64, _p, _p, _i64, _int, _int, _p, _i64, _p, _p, _p, _sz, _p]),
    "gn_rgcn_plan_build_positions": (_int, [_p, _p, _p, _p]),
    "gn_rgcn_weighted_supported": (_int, [_p, _i64, _i64, _i64]),
    "gn_rgcn_weighted_workspace_bytes": (_sz, [_p, _i64, _i64, _i64]),
    "gn_rgcn_forward_weighted_f32": (_int, [_p, _p, _i64, _i64, _p, _p, _i64, _p, _p, _i64, _int, _int, _p, _p, _i64, _p, _sz, _p]),
    "gn_rgcn_weight_grad_weighted_f32": (_int, [_p, _p, _p, _p, _p, _i64, _i64, _p, _i64, _i64, _p, _p, _sz, _p]),
    "gn_rgcn_finalize_f32": (_int, [_p, _p, _i64, _p, _i64, _i64, _p, _p, _i64, _int, _p, _i64, _p, _p]),
    "gn_distmult_forward_f32": (_int, [_p, _i64, _i64, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _int, _p, _p, _p]),
    "gn_distmult_packed_forward_f32": (_int, [_p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _int, _p, _p, _p]),
    "gn_distmult_plan_create": (_int, [_p, _p, _p, _i64, _i64, _i64, _i64, _p, C.POINTER(_p)]),
    "gn_distmult_plan_destroy": (None, [_p]),
    "gn_distmult_plan_edges": (_i64, [_p]),
    "gn_distmult_plan_forward_f32": (_int, [_p, _p, _i64, _i64, _p, _i64, _int, _p, _p]),
    "gn_distmult_plan_forward_cols_f32": (_int, [_p, _p, _i64, _i64, _i64, _i64, _p, _i64, _int, _p, _p]),
    "gn_xtg_workspace_bytes": (_sz, [_i64, _i64]),
    "gn_xtg_f32": (_int, [_p, _i64, _p, _i64, _i64, _i64, _i64, _p, _i64, _p, _sz, _int, _p]),
    "gn_distmult_backward_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "gn_dense_batch_begin": (_int, []),
    "gn_dense_batch_end": (_int, [_p]),
    "gn_distmult_type_tasks_bytes": (_sz, [_i64, _i64]),
    "gn_distmult_type_tasks": (_int, [_p, _i64, _i64, _p, _sz, _p]),
    "gn_distmult_backward_f32": (_int, [_p, _i64, _i64, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _i64, _p, _i64, _p, _sz, _p]),
    "gn_distmult_backward_ex_f32": (_int, [_p, _i64, _i64, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _p, _p, _i64, _p, _i64, _int, _p, _p, _p, _sz, _p]),
    "gn_distmult_backward_packed_f32": (_int, [_p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _p, _p, _i64, _p, _i64, _int, _p, _p, _p, _sz, _p]),
    "gn_distmult_bwd_plan_create": (_int, [_p, _p, _p, _i64, _i64, _i64, _p, C.POINTER(_p)]),
    "gn_distmult_bwd_plan_destroy": (None, [_p]),
    "gn_distmult_bwd_plan_workspace_bytes": (_sz, [_p, _i64]),
    "gn_distmult_backward_planned_f32": (_int, [_p, _p, _i64, _i64, _p, _i64, _p, _p, _p, _i64, _p, _i64, _p, _sz, _p]),
    "gn_distmult_backward_loss_packed_f32": (_int, [_p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _p, _i64, _int, _p, _p, _i64, _p, _i64, _p, _sz, _p]),
    "gn_distmult_backward_loss_planned_f32": (_int, [_p, _p, _i64, _i64, _p, _i64, _p, _p, _p, _i64, _p, _i64, _p, _sz, _p]),
    "gn_kge_forward_workspace_bytes": (_sz, [_int, _i64, _i64]),
    "gn_kge_forward_f32": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, C.c_float, C.c_float, _int, _p, _p, _p, _p, _sz, _p]),
    "gn_kge_backward_workspace_bytes": (_sz, [_int, _i64, _i64, _i64, _i64]),
    "gn_kge_backward_f32": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, C.c_float, _p, _p, _p, _i64, _p, _i64, _int, _p, _sz, _p]),
    "gn_kge_batch_forward_workspace_bytes": (_sz, [_int, _i64, _i64]),
    "gn_kge_batch_forward_f32": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _int, C.c_float, C.c_float, _int, _p, _p, _p, _p, _sz, _p]),
    "gn_kge_batch_backward_workspace_bytes": (_sz, [_int, _i64, _i64, _i64, _i64, _i64]),
    "gn_kge_batch_backward_f32": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _int, C.c_float, _p, _p, _p, _i64, _p, _i64, _int, _p, _sz, _p]),
    "gn_kge_shared_forward_workspace_bytes": (_sz, [_int, _i64, _i64]),
    "gn_kge_shared_forward_f32": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _int, C.c_float, C.c_float, _int, _p, _p, _p, _p, _sz, _p]),
    "gn_kge_shared_backward_workspace_bytes": (_sz, [_int, _i64, _i64, _i64, _i64, _i64, _i64]),
    "gn_kge_shared_backward_f32": (_int, [_int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, _i64, _i64, _i64, _int, C.c_float, _p, _p, _p, _i64, _p, _i64, _int, _p, _sz, _p]),
    "gn_kge_ns_loss_workspace_bytes": (_sz, [_i64]),
    "gn_kge_ns_loss_forward_f32": (_int, [_p, _p, _i64, _i64, _i64, _p, _int, C.c_float, _p, _p, _p, _p, _sz, _p]),
    "gn_kge_ns_loss_backward_f32": (_int, [_p, _p, _i64, _i64, _i64, _p, _int, C.c_float, _p, _p, _p, _p, _p, _i64, _p]),
    "gn_kge_candidates_sample": (_int, [_p, _p, _i64, _i64, _i64, _i64, _p, C.c_uint64, _p, _p, _i64, _p, _p]),
    "gn_kge_candidates_sample_ranged": (_int, [_p, _p, _i64, _i64, _i64, _i64, _p, C.c_uint64, _p, _p, _i64, _p, _p, _p]),
    "gn_gat_logits_f32": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _p, _p]),
    "gn_gat_forward_f32": (_int, [_p, _p, _i64, _i64, _i64, _p, _p, C.c_float, _p, _int, _int, _p, _i64, _p, _p, _p, _p]),
    "gn_gat_backward_dst_f32": (_int, [_p, _p, _i64, _i64, _i64, _p, _p, _p, _p, C.c_float, _p, _i64, _int, _p, _p, _p, _p]),
    "gn_gat_backward_src_f32": (_int, [_p, _p, _i64, _i64, _i64, _p, _p, C.c_float, _p, _i64, _int, _p, _p, _p, _i64, _p, _p]),
    "gn_gat_att_grad_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "gn_gat_att_grad_f32": (_int, [_p, _i64, _i64, _i64, _i64, _p, _p, _p, _p, _sz, _p]),
    "gn_kge_rank_workspace_bytes": (_sz, [_int, _i64, _i64, _i64]),
    "gn_kge_rank_f32": (_int, [_int, _int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, C.c_float, C.c_float, _p, _p, _p, _p, _p, _sz, _p]),
    "gn_kge_topk_f32": (_int, [_int, _int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _i64, _i64, C.c_float, C.c_float, _p, _p, _p, _p, _p, _sz, _p]),
    "gn_kge_rank_ranged_f32": (_int, [_int, _int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _p, _i64, C.c_float, C.c_float, _p, _p, _p, _p, _p, _sz, _p, _p]),
    "gn_kge_topk_ranged_f32": (_int, [_int, _int, _p, _i64, _i64, _p, _i64, _i64, _i64, _p, _p, _i64, _i64, C.c_float, C.c_float, _p, _p, _p, _p, _p, _sz, _p, _p]),
    "gn_negative_sampler_create": (_int, [_p, _p, _p, _i64, _i64, _i64, _p, C.POINTER(_p)]),
    "gn_negative_sampler_destroy": (None, [_p]),
    "gn_negative_sampler_sample": (_int, [_p, C.c_uint64, _p, _p, _p, _p]),
    "gn_negative_sampler_sample_packed": (_int, [_p, C.c_uint64, _p, _p, _p, _p, _p]),
    "gn_negative_sampler_sample_stepped": (_int, [_p, C.c_uint64, _p, _p, _p, _p, _p, _p]),
    "gn_known_pairs_create": (_int, [_p, _p, _p, _i64, _i64, _i64, _p, C.POINTER(_p)]),
    "gn_known_pairs_destroy": (None, [_p]),
    "gn_distmult_rank_f32": (_int, [_p, _i64, _i64, _i64, _p, _i64, _i64, _p, _p, _p, _i64, _p, _p, _p, _p, _p]),
    "gn_distmult_topk_f32": (_int, [_p, _i64, _i64, _i64, _p, _i64, _i64, _p, _p, _i64, _i64, _p, _p, _p, _p, _p]),
    "gn_distmult_rank_ranged_f32": (_int, [_p, _i64, _i64, _i64, _p, _i64, _i64, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _p]),
    "gn_distmult_topk_ranged_f32": (_int, [_p, _i64, _i64, _i64, _p, _i64, _i64, _p, _p, _i64, _i64, _p, _p, _p, _p, _p, _p]),
    "gn_rgcn_weight_grad_workspace_bytes": (_sz, [_p, _i64, _i64]),
    "gn_rgcn_weight_grad_supported": (_int, [_p, _i64, _i64]),
    "gn_rgcn_weight_grad_f32": (_int, [_p, _p, _p, _p, _i64, _i64, _p, _i64, _i64, _p, _p, _sz, _p]),
    "gn_rel_grad_plan_create": (_int, [_p, _i64, _i64, _p, C.POINTER(_p)]),
    "gn_rel_grad_plan_destroy": (None, [_p]),
    "gn_rel_weight_grad_supported": (_int, [_p, _i64, _i64]),
    "gn_rel_weight_grad_f32": (_int, [_p, _p, _i64, _i64, _p, _i64, _i64, _p, _p]),
    "gn_grad_prologue_workspace_bytes": (_sz, []),
    "gn_grad_prologue_f32": (_int, [_p, _i64, _p, _i64, _p, _i64, _i64, _p, _i64, _p, _i64, _p, _p, _sz, _p]),
    "gn_adam_step_f32": (_int, [_p, _int, _p, _p, _sz, C.c_float, C.c_double, C.c_double, C.c_float, C.c_float, _p]),
    "gn_class_loss_forward_f32": (_int, [_p, _i64, _p, _i64, _i64, C.c_float, _p, _p, _p]),
    "gn_class_loss_backward_f32": (_int, [_p, _i64, _p, _i64, _i64, C.c_float, _p, _p, _i64, _p]),
    "gn_link_loss_workspace_bytes": (_sz, []),
    "gn_link_loss_forward_f32": (_int, [_p, _i64, _p, _i64, C.c_float, _p, _p, _sz, _p]),
    "gn_link_loss_backward_f32": (_int, [_p, _i64, _p, _i64, C.c_float, _p, _p, _p, _p]),
    "gn_exchange_buffer_bytes": (_sz, [_i64, _int]),
    "gn_exchange_push_f32": (_int, [_p, _i64, _p, _p, _p, _int, _int, _int, _p]),
    "gn_exchange_wait_sum_f32": (_int, [_p, _p, _i64, _int, _int, _p, _int, _p, _p]),
    "gn_link_metrics_plan_create": (_int, [_p, _i64, _i64, _p, C.POINTER(_p)]),
    "gn_link_metrics_plan_destroy": (None, [_p]),
    "gn_link_metrics_plan_workspace_bytes": (_sz, [_p]),
    "gn_link_metrics_planned_f32": (_int, [_p, _p, _p, _p, _p, _sz, _p]),
    "gn_link_metrics_workspace_bytes": (_sz, [_i64, _i64]),
    "gn_link_metrics_f32": (_int, [_p, _p, _p, _i64, _i64, _p, _p, _sz, _p]),
    "gn_class_metrics_workspace_bytes": (_sz, [_i64, _i64]),
    "gn_class_metrics_f32": (_int, [_p, _i64, _p, _p, _i64, _i64, _p, _p, _p, _p, _p, _p, _sz, _p]),
}


class AdamTensor(C.Structure):
    """gn_adam_tensor of include/gripnet_hip.h."""
    _fields_ = [("param", _p), ("grad", _p), ("exp_avg", _p), ("exp_avg_sq", _p), ("numel", _i64)]


class SideCopy(C.Structure):
    """gn_side_copy: a concat slot filled by the launch that produces its neighbour slot."""
    _fields_ = [("src", _p), ("ld_src", _i64), ("dst", _p), ("ld_dst", _i64), ("rows", _i64), ("cols", _i64),
                ("mode", _int)]


def side_copy(spec):
    """spec = (src, dst, mode) of 2-D fp32 tensors with equal shapes, or None."""
    if spec is None:
        return None
    src, dst, mode = spec
    src = f32_rows(src)
    if tuple(src.shape) != tuple(dst.shape):
        raise ValueError("side copy shapes differ: {} vs {}".format(tuple(src.shape), tuple(dst.shape)))
    sc = SideCopy(src.data_ptr(), ld(src), dst.data_ptr(), ld(dst), src.shape[0], src.shape[1], int(mode))
    sc._keep = (src, dst)
    return sc


class SplitPlanesDesc(C.Structure):
    """gn_split_planes: where a launch leaves the bf16 split planes of what it writes."""
    _fields_ = [("planes", _p), ("rows", _i64), ("nt", _int), ("col_main", _int), ("col_side", _int)]


class SplitPlanes:
    """The bf16 split planes of a row-major fp32 matrix X [rows, 16 nt] (x = hi + mid + lo exactly): what the
    relational layer's matrix products run on, left behind by the layer that produces X (gn_split_planes in
    include/gripnet_hip.h).  Owns the buffer; its last row stays zero."""

    def __init__(self, rows: int, nt: int, device):
        self.rows, self.nt, self.device = int(rows), int(nt), device
        self.buf = torch.zeros((int(load().gn_split_planes_bytes(self.rows, self.nt)),), dtype=torch.uint8, device=device)
        self.generation = 0          # bumped by every launch that rewrites the planes

    def desc(self, col_main=0, col_side=0):
        d = SplitPlanesDesc(self.buf.data_ptr(), self.rows, self.nt, int(col_main), int(col_side))
        d._keep = self.buf
        return d

    def fill_from(self, x: torch.Tensor):
        """Stand-alone split of an existing matrix (callers without a producing layer)."""
        d = self.desc()
        _call("gn_split_planes_f32", ptr(x), ld(x), x.shape[0], x.shape[1], 0, C.byref(d), stream_ptr(x.device))
        self.generation += 1
        return self

    def tag(self, x: torch.Tensor):
        """Remember on `x` that these planes hold its current contents."""
        x._gn_planes = (self, self.generation, x._version)
        return x

    def rewritten_for(self, x: torch.Tensor):
        """A launch rewrote the planes with the contents of `x`: they describe `x` (and nothing tagged before) now."""
        self.generation += 1
        return self.tag(x)

    @staticmethod
    def of(x: torch.Tensor, nt: int):
        """The planes tagged on `x`, if they still describe it (same tensor version, not rewritten since), else None."""
        t = getattr(x, "_gn_planes", None)
        if t is None:
            return None
        planes, gen, ver = t
        if planes.generation != gen or x._version != ver or planes.nt != nt or planes.rows != x.shape[0] or planes.device != x.device:
            return None
        return planes


def _ref(sc):
    return None if sc is None else C.byref(sc)


class GripNetHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


class Unsupported(GripNetHipError):
    """GN_ERR_UNSUPPORTED: the library refused this path for these shapes or alignments - the caller takes the next one."""


def library_path() -> str:
    return _LIB_PATH


def load():
    """Load the shared library once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(_LIB_PATH):
                raise RuntimeError(
                    "gripnet_amd: {} is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(or `make -C gripnet_amd/csrc`). There is no CPU fallback.".format(_LIB_PATH))
            lib = C.CDLL(_LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            if lib.gn_version() < ABI_VERSION:
                raise RuntimeError("gripnet_amd: libgripnet_hip.so is older than this package")
            _lib = lib
    return _lib


def check(status: int):
    if status == GN_OK:
        return
    msg = load().gn_last_error().decode("utf-8", "replace")
    if status == GN_ERR_INDEX_RANGE:
        raise IndexError(msg)
    if status == GN_ERR_INVALID_ARG:
        raise ValueError(msg)
    if status == GN_ERR_UNSUPPORTED:
        raise Unsupported(status, msg)
    raise GripNetHipError(status, msg)


class KernelTimer:
    """Optional per-entry-point device timing: while active, every launch made through this
    module is bracketed by HIP events on the launching stream (used by bench.py's roofline)."""

    def __init__(self, only=None, pool=0, every=1, records_only=False):
        """`pool`: events created (and recorded once, which is when HIP allocates them) up front, so that a timed
        region pays two event records per bracketed launch and nothing else.  `every`: bracket only every n-th launch
        of an entry point (an event record costs ~4.5 us of stream time on this stack: two per step are 9 % of a 95 us
        step; a sample of the launches gives the same average duration)."""
        self.events = {}
        self.records_only = bool(records_only)      # never the kernels' own dispatch stamps (gn_time_next_launch)
        self.every, self._seen = max(1, int(every)), {}
        self.only = None if only is None else set(only)
        self._pool = [torch.cuda.Event(enable_timing=True) for _ in range(pool)]
        for e in self._pool:
            e.record()

    def event(self):
        return self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        global _timer
        self._prev, _timer = _timer, self
        return self

    def __exit__(self, *exc):
        global _timer
        _timer = self._prev

    def add(self, name, start, stop):
        self.events.setdefault(name, []).append((start, stop))

    def summary(self):
        """name -> (calls, total_ms); synchronises."""
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in self.events.items()}


_timer = None

# Entry points whose kernel can carry its own start / stop events (gn_time_next_launch): no marker packets in the stream.  An
# entry point that turns out to launch another kernel (the events stay pending) is timed with event records from then on.
_STAMPED = {"gn_rgcn_forward_f32", "gn_distmult_plan_forward_f32"}


def _timed_call(t, fn, args, name, tag):
    """One bracketed call under KernelTimer `t`: the kernel's own dispatch stamps where the entry point supports them,
    else an event record in front of and behind the launch (each ~4.5 us of stream time on this stack)."""
    start, stop = t.event(), t.event()
    if name in _STAMPED and not t.records_only and start.cuda_event and stop.cuda_event:      # (a pooled event: its handle exists)
        lib = load()
        lib.gn_time_next_launch(start.cuda_event, stop.cuda_event)
        status = fn(*args)
        if lib.gn_time_launch_pending():                  # another kernel served the call: untimed this once, records from now on
            _STAMPED.discard(name)
            t._pool.extend((start, stop))
        else:
            t.add(tag or name, start, stop)
        return status
    start.record()
    status = fn(*args)
    stop.record()
    t.add(tag or name, start, stop)
    return status


class Recorder:
    """While active, every entry-point call made through this module is also written down - (bound C function, arguments,
    name, tag) - and the tensors whose pointers it was given are held, so that `replay` can make the same calls again straight
    from a loop, without the Python layers above them (module forward, plan look-up, pointer extraction: ~15 us per entry
    point against ~4 us for the call itself).  The calls launch on the stream that was current when they were recorded and
    read / write the buffers they were recorded with, like a captured hipGraph - but a replay is ordinary launches: it
    pipelines behind whatever the stream is still running, where a graph launch on this stack leaves the GPU idle for
    ~9 us in front of its first kernel (tools/launch_modes.py, profiles/r04_counters.md)."""

    def __init__(self):
        self.calls, self.keep = [], []

    def __enter__(self):
        global _recorder
        self._prev, _recorder = _recorder, self
        return self

    def __exit__(self, *exc):
        global _recorder
        _recorder = self._prev


_recorder = None


def replay(calls):
    """Make recorded calls again, in order; an active KernelTimer brackets the ones it names (sampled as in _call)."""
    t = _timer
    for fn, args, name, tag in calls:
        if t is not None and (t.only is None or name in t.only):
            seen = t._seen.get(name, 0)
            t._seen[name] = seen + 1
            if seen % t.every == 0:
                status = _timed_call(t, fn, args, name, tag)
                if status:
                    check(status)
                continue
        status = fn(*args)
        if status:
            check(status)


# Test hooks the library reads from the environment at call time (common.h, aggregate.cuh, gcn_blocked.hip): part of every
# memo key, so that a shortcut recorded under one setting is not replayed under another.
_ENV_HOOKS = ("GN_DISABLE_FAST", "GN_DISABLE_QUAD", "GN_DISABLE_BLOCKED", "GN_BLOCKED_ANY", "GN_DISABLE_LDS_TABLE",
              "GN_ENABLE_CHAIN", "GN_BLOCKED_DIRECT")
# hooks the C side reads that can NOT change what a memoised inference forward launches: the host threads of the plan builders
# (plans do not depend on them), the sampler's kernel choice (same draws; no module forward calls the sampler) and the slab size of the
# general relational path (read inside the entry point at every call: a slab is a range of rows, the bits do not depend on it).
# tests/test_abi.py::test_env_hooks_cover_the_library holds the two lists to the getenv calls of csrc/.
_ENV_NEUTRAL = ("GN_PLAN_THREADS", "GN_SAMPLER_TASKS", "GN_RGCN_SLAB_MB")
_ENV_DATA = getattr(os.environ, "_data", None)
_ENV_KEYS = tuple(k.encode() for k in _ENV_HOOKS) if isinstance(_ENV_DATA, dict) and all(isinstance(k, bytes) for k in list(_ENV_DATA)[:1]) else None


def release_host_scratch() -> int:
    """Give the plan builders' kept block of host memory back to the system (gn_host_scratch_release); the bytes freed."""
    return int(load().gn_host_scratch_release())


def device_blocks_live() -> int:
    """Device allocations the library holds right now (gn_device_blocks_live): plan buffers plus builders' scratch blocks."""
    return int(load().gn_device_blocks_live())


def env_stamp():
    """The current values of the library's environment hooks (plain dict look-ups on CPython's POSIX `os.environ`)."""
    if _ENV_KEYS is not None:
        d = _ENV_DATA
        return tuple([d.get(k) for k in _ENV_KEYS])
    return tuple([os.environ.get(k) for k in _ENV_HOOKS])


def launch_context(device):
    """(current device, raw stream) a memoised call sequence is bound to."""
    index = device.index
    return torch.cuda.current_device(), (_raw_stream(index) if _raw_stream is not None else torch.cuda.current_stream(index).cuda_stream)


class CallMemo:
    """Steady-state shortcut of ONE module's inference forward (the reference-shaped API of layers.py / decoder.py as a
    caller of GripNet-pose.py:117-138 uses it): the C-ABI calls a forward makes are a function of a few pointers, shapes
    and versions - the module computes that key, and when the key repeats the calls are made again straight from the
    recording (`replay`), without the Python between the module's `forward` and the library (~20 us per entry point:
    module dispatch, plan look-ups, layout checks, ctypes structures).  The OUTPUT is allocated fresh by the module on
    every call (the reference returns fresh tensors) and its address is part of the key: under torch's caching allocator
    a loop's outputs cycle through one or two addresses.  A key is recorded the second time in a row it is seen (one-shot
    inputs - fresh negative samples - never fill the table).  An entry keeps alive what its calls read besides the
    caller's input and the output (plans' scratch, temporaries the slow path allocated, the by-reference structures), and
    what the module's `hold` names: every object whose `id` is part of the key, so that no id is reused under a live
    recording."""

    DEPTH = 8

    def __init__(self):
        self.entries = {}                    # key -> (calls, keep, post)
        self.last = None

    @classmethod
    def of(cls, module):
        """The memo of `module` (`module.__dict__["_memo"]`: not a submodule, not in the state dict), made at first use."""
        memo = module.__dict__.get("_memo")
        if memo is None:
            memo = module.__dict__["_memo"] = cls()
        return memo

    def run(self, guard, out, run, drop, hold, post=None):
        """One forward whose calls are a function of `guard` and the address of `out`.  Recorded already: the calls again,
        then what the recording's `post()` gave (None, or a callable) with `out`.  Else `run()`, and when `guard` was also
        the previous call's, with every entry-point call written down and stored; `drop`: tensors (the caller's input, the
        fresh output) the entry must NOT keep alive; `hold()`: objects it must, asked AFTER the run (a plan may only exist then)."""
        key = guard + (out.data_ptr(),)
        hit = self.entries.get(key)
        if hit is not None:
            replay(hit[0])
            if hit[2] is not None:
                hit[2](out)
            return out
        seen, self.last = self.last == guard, guard
        if not seen or _recorder is not None:
            return run()
        drop_ptrs = {t.untyped_storage().data_ptr() for t in drop if t is not None}
        with Recorder() as rec:
            result = run()
        keep = list(hold())
        for item in rec.keep:
            if torch.is_tensor(item):
                if item.untyped_storage().data_ptr() not in drop_ptrs:
                    keep.append(item)
                continue
            if isinstance(item, tuple):      # an argument tuple: its by-reference structures stay, what THEY held is filtered too
                for a in item:
                    obj = getattr(a, "_obj", None)
                    held = getattr(obj, "_keep", None) if obj is not None else None
                    if held is not None:
                        for t in (held if isinstance(held, tuple) else (held,)):
                            if torch.is_tensor(t) and t.untyped_storage().data_ptr() not in drop_ptrs:
                                keep.append(t)
                        obj._keep = None
            keep.append(item)
        while len(self.entries) >= self.DEPTH:
            self.entries.pop(next(iter(self.entries)))
        self.entries[key] = (rec.calls, keep, None if post is None else post())
        return result


def _call(name, *args, tag=None):
    """Call an entry point.  Every caller passes `stream_ptr(<device of its operands>)` among the arguments; when that
    device is not the current one the call is made with it current (a launch on a foreign device's stream fails or
    lands on the wrong device)."""
    global _stream_device
    fn = getattr(load(), name)
    dev, _stream_device = _stream_device, None
    if dev is not None and dev != torch.cuda.current_device():
        with torch.cuda.device(dev):
            return _call(name, *args, tag=tag)
    t = _timer
    timed = t is not None and (t.only is None or name in t.only)
    if timed and t.every > 1:
        seen = t._seen.get(name, 0)
        t._seen[name] = seen + 1
        timed = seen % t.every == 0
    if timed:
        status = _timed_call(t, fn, args, name, tag)
    else:
        status = fn(*args)
    check(status)
    if _recorder is not None:                        # (calls that were refused - a path that does not apply - are not part of the recording)
        _recorder.calls.append((fn, args, name, tag))
        _recorder.keep.append(args)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "gripnet_amd runs on an MI355X only: got a {} tensor on {} (no CPU fallback; "
                "move the model and the data to 'cuda')".format(tuple(t.shape), t.device))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_stream_device = None       # device index of the last stream_ptr(): read (and cleared) by _call


def stream_ptr(device=None) -> int:
    """hipStream_t of torch's current stream on `device` (the raw getter costs a fraction of building a Stream object;
    eager launching of the ~120 us forward is close to host-bound)."""
    global _stream_device
    index = device.index if isinstance(device, torch.device) else device
    if index is None:
        index = torch.cuda.current_device()
    _stream_device = index
    if _raw_stream is not None:
        return _raw_stream(index)
    return torch.cuda.current_stream(index).cuda_stream


def f32_rows(t: torch.Tensor) -> torch.Tensor:
    """fp32 2-D view whose rows are contiguous (any row stride); copies only if it must."""
    if t.dtype != torch.float32:
        raise TypeError("gripnet_amd computes in fp32; got {}".format(t.dtype))
    if t.dim() != 2:
        raise ValueError("expected a 2-D feature matrix, got shape {}".format(tuple(t.shape)))
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def i64_vec(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.int64:
        raise TypeError("indices must be int64 (torch.long), got {}".format(t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def edge_rows(edge_index: torch.Tensor):
    """(tensor kept alive, src pointer, dst pointer, E) of a [2, E] int64 edge_index."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must have shape [2, E], got {}".format(tuple(edge_index.shape)))
    ei = i64_vec(edge_index)
    e = int(ei.shape[1])
    base = ei.data_ptr()
    return ei, base, base + 8 * e, e


def transform_fusable(fin: int, fout: int, x: torch.Tensor) -> bool:
    """True when gn_graph_aggregate_f32 can contract with W in its epilogue for this input."""
    return bool(load().gn_transform_fusable(int(fin), int(fout))) and ld(x) % 4 == 0 and x.data_ptr() % 16 == 0


def e_count(edge_index):
    return int(edge_index.shape[1])


def ptr(t):
    if t is None:
        return None
    if _recorder is not None:
        _recorder.keep.append(t)             # a recorded call's operands stay alive as long as the recording
    return t.data_ptr()


# ---- thin typed wrappers ---------------------------------------------------------------------
def gemm(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, bias=None, relu=False, a_rows=None,
         batch=1, stride_a=0, stride_b=0, stride_c=0, m=None, n=None, k=None, lda=None, ldb=None, ldc=None, fast=False,
         b_transposed=False, accumulate=False, a_transposed=False, join_batch=False, addend=None, out_bf16=False):
    """`join_batch`: inside ``with dense_batch(...)`` the product may be queued and leave with the batch (it must not depend
    on another queued product).  `fast`: two-term bf16 splits (<= 2^-16 per product) instead of the default fp32-faithful arithmetic.
    `b_transposed`: b is [n, k] (out = a b^T); `a_transposed`: a is [k, m] (out = a^T b; m <= 64 or n <= 32 only);
    `accumulate`: out += a b; `addend`: an [m, n] fp32 matrix (rows contiguous, any row stride) added to what is stored
    (gn_gemm_addend_f32) - the other gradient of a tensor with two consumers, see `addend_ok`.  `out_bf16`: `out` is a bf16
    table, every value rounded once where it is stored (GN_GEMM_OUT_BF16; raises Unsupported for shapes outside the
    tall-skinny kernel)."""
    if a_transposed:
        m = a.shape[1] if m is None else m
        k = a.shape[0] if k is None else k
    m = (a.shape[0] if a_rows is None else a_rows.shape[0]) if m is None else m
    k = a.shape[1] if k is None else k
    n = (b.shape[0] if b_transposed else b.shape[-1]) if n is None else n
    join_batch = join_batch and getattr(_batch_tls, 'open', None) is not None
    if join_batch:                                           # a queued product reads its operands when the batch leaves
        _batch_tls.open.keep.extend((a, b, out, bias, a_rows, addend))
    flags = ((GN_GEMM_RELU if relu else 0) | (GN_GEMM_ARITH_FAST if fast else 0) | (GN_GEMM_B_TRANSPOSED if b_transposed else 0) |
             (GN_GEMM_ACCUMULATE if accumulate else 0) | (GN_GEMM_A_TRANSPOSED if a_transposed else 0) | (GN_GEMM_JOIN_BATCH if join_batch else 0) |
             (GN_GEMM_OUT_BF16 if out_bf16 else 0))
    head = (ptr(a), ld(a) if lda is None else lda, stride_a, ptr(a_rows), a.shape[0],
            ptr(b), ld(b) if ldb is None else ldb, stride_b,
            ptr(out), ld(out) if ldc is None else ldc, stride_c, m, n, k, batch, ptr(bias))
    if addend is None:
        _call("gn_gemm_f32", *head, flags, stream_ptr(a.device))
    else:
        if not addend_ok(addend, m, n) or batch != 1:
            raise ValueError("addend: an fp32 [m, n] matrix with contiguous rows, single product")
        _call("gn_gemm_addend_f32", *head, ptr(addend), ld(addend), flags, stream_ptr(a.device))
    return out


def addend_ok(t, m, n) -> bool:
    """Can `t` ride on a product's store as its addend?  (fp32, [m, n], unit column stride - a column slice of a concat's gradient is)"""
    return (t is not None and t.dtype == torch.float32 and t.dim() == 2 and tuple(t.shape) == (m, n) and t.is_cuda and
            (n == 1 or t.stride(1) == 1) and (m == 1 or t.stride(0) >= n))


_zeroed = {}        # (device type, device index, what) -> a buffer filled with zeros when it was made


def zeroed_once(device, what, numel, dtype=torch.uint8):
    """The buffer `what` of `device`, zeroed once: scratch whose kernels leave it ready for the next launch, and the error
    words.  `numel`: its length, or a function that is asked for it when the buffer is made."""
    key = (device.type, device.index, what)
    buf = _zeroed.get(key)
    if buf is None:
        buf = _zeroed[key] = torch.zeros((int(numel() if callable(numel) else numel),), dtype=dtype, device=device)
    return buf


GN_XTG_TICKET_ZEROED, GN_XTG_JOIN_BATCH = 1, 2


def xtg(x: torch.Tensor, g: torch.Tensor, join_batch=False):
    """x^T g for a tall x [m, k1] and g [m, k2] (weight gradients) on gn_xtg_f32: up to 64 x 32 outputs in one launch; wider
    products (the 128 x 64 ... 256 x 128 layers of the node-classification models) as wide products of up to 256 x 128 outputs
    (a launch + a fold) where the sizes allow, else in tiles of 64 x 32 outputs over column slices of x and g; every block
    with a workspace of its own.  `join_batch`: as in `gemm`."""
    k1, k2 = x.shape[1], g.shape[1]
    out = torch.empty((k1, k2), dtype=torch.float32, device=x.device)
    if k1 * k2 == 0:
        return out
    if x.shape[0] == 0:
        return out.zero_()
    if k1 <= 64 and k2 <= 32:
        tiles = [(0, k1, 0, k2)]
    else:
        # blocks of up to 256 x 128 outputs that gn_xtg_f32 takes as ONE wide product (x and g read once); what is left, in
        # tiles of 64 x 32
        tiles, lib, m = [], load(), x.shape[0]
        for c0 in range(0, k1, 256):
            for d0 in range(0, k2, 128):
                w1, w2 = min(256, k1 - c0), min(128, k2 - d0)
                if lib.gn_xtg_wide_supported(m, w1, w2):
                    tiles.append((c0, w1, d0, w2))
                else:
                    tiles.extend((c0 + a, min(64, w1 - a), d0 + b, min(32, w2 - b)) for a in range(0, w1, 64) for b in range(0, w2, 32))
    batched = join_batch and getattr(_batch_tls, 'open', None) is not None
    for t, (c0, w1, d0, w2) in enumerate(tiles):
        need = int(load().gn_xtg_workspace_bytes(w1, w2))
        ws = zeroed_once(x.device, ("xtg", need, t), need)     # one zeroed workspace per device, size and tile: its last 64 bytes are the kernel's ticket
        xs, gs, os_ = (x, g, out) if len(tiles) == 1 else (x[:, c0:c0 + w1], g[:, d0:d0 + w2], out[c0:c0 + w1, d0:d0 + w2])
        if batched:
            _batch_tls.open.keep.extend((xs, gs, os_))
        _call("gn_xtg_f32", ptr(xs), ld(xs), ptr(gs), ld(gs), x.shape[0], w1, w2, ptr(os_), ld(os_), ptr(ws), need,
              GN_XTG_TICKET_ZEROED | (GN_XTG_JOIN_BATCH if batched else 0), stream_ptr(x.device))
    return out


def grad_prologue(g, saved_out=None, rowdiv=None, want_masked=True, want_colsum=False):
    """(gm, gd, colsum) of gn_grad_prologue_f32: gm = g masked by saved_out > 0 (None when not wanted), gd = gm / rowdiv
    (None without rowdiv), colsum = the column sums of gm (None when not wanted).  `g` may be a row-strided view."""
    g = f32_rows(g)
    rows, cols = g.shape
    dev = g.device
    gm = torch.empty((rows, cols), dtype=torch.float32, device=dev) if want_masked else None
    gd = torch.empty((rows, cols), dtype=torch.float32, device=dev) if rowdiv is not None else None
    cs = torch.empty((cols,), dtype=torch.float32, device=dev) if want_colsum else None
    ws = zeroed_once(dev, "grad prologue", load().gn_grad_prologue_workspace_bytes) if want_colsum else None
    _call("gn_grad_prologue_f32", ptr(g), ld(g), ptr(saved_out), 0 if saved_out is None else ld(saved_out), ptr(rowdiv), rows, cols,
          ptr(gm), cols, ptr(gd), cols, ptr(cs), ptr(ws), 0 if ws is None else ws.numel(), stream_ptr(dev))
    return gm, gd, cs


def merge(dst: torch.Tensor, src: torch.Tensor, mode: int, src2=None):
    _call("gn_merge_f32", ptr(dst), ld(dst), ptr(src), ld(src), ptr(src2), 0 if src2 is None else ld(src2),
          dst.shape[0], dst.shape[1], mode, stream_ptr(dst.device))
    return dst


class Handle:
    """Owner of one handle of the library (`_h`): made by `_create`, given back by the entry point `_destroy` names when
    the object goes - once, never after the module has let go of the library, and never for an object whose creation raised
    (its `_h` is still the class's None)."""
    _h = None
    _destroy = None

    def _create(self, name, device, *args):
        """`_h` = the handle that entry point `name` makes of `args` (then the stream and the handle's address, as every
        create entry point ends), with `device` current."""
        h = _p()
        with torch.cuda.device(device):
            check(getattr(load(), name)(*args, stream_ptr(device), C.byref(h)))
        self._h = h

    def __del__(self):
        h, self._h = self._h, None
        if h and _lib is not None:
            getattr(_lib, self._destroy)(h)


class GraphPlan(Handle):
    """Owner of a gn_graph_plan handle (the cached normalised graph of one GCN-style layer)."""
    _destroy = "gn_graph_plan_destroy"

    def __init__(self, handle, device, kind):
        self._h, self.device, self.kind = handle, device, kind
        self._export = None

    @classmethod
    def _build(cls, kind, create, edge_index, edge_weight, n_table, n_rows, size_a, size_b):
        """The plan `create` makes of (sources, destinations, weights or None, E, size_a, size_b)."""
        load()
        require_gpu(edge_index, edge_weight)
        ei, src, dst, e = edge_rows(edge_index)
        w = None if edge_weight is None else edge_weight.to(torch.float32).contiguous()
        if w is not None and w.numel() != e:
            raise ValueError("edge_weight has {} entries for {} edges".format(w.numel(), e))
        plan = cls(None, ei.device, kind)
        plan._create(create, ei.device, src, dst, ptr(w), e, int(size_a), int(size_b))
        plan.n_rows, plan.n_table = int(n_rows), int(n_table)
        return plan

    @classmethod
    def gcn(cls, edge_index, num_nodes, edge_weight=None, improved=False):
        return cls._build("gcn", "gn_gcn_plan_create", edge_index, edge_weight, num_nodes, num_nodes, num_nodes, bool(improved))

    @classmethod
    def bipartite(cls, edge_index, num_sources, num_targets, edge_weight=None):
        return cls._build("bipartite", "gn_bipartite_plan_create", edge_index, edge_weight, num_sources, num_targets,
                          num_sources, num_targets)

    @classmethod
    def plain_sum(cls, edge_index, num_sources, num_targets):
        """out[t] = sum of table[s] over the edges s -> t (no normalisation)."""
        return cls._build("sum", "gn_sum_plan_create", edge_index, None, num_sources, num_targets, num_sources, num_targets)

    def build_blocked(self, cols: int):
        """Add the source-blocked encoding (LDS-staged gathers) for rows of up to `cols` floats; a no-op for
        graphs that do not qualify.  Returns the width the plan covers (0: wave-per-row kernels)."""
        if self.kind == "gcn" and cols <= 32:
            with torch.cuda.device(self.device):
                check(load().gn_graph_plan_build_blocked(self._h, 16 if cols <= 16 else 32, stream_ptr(self.device)))
        return self.blocked_cols

    @property
    def blocked_cols(self) -> int:
        return int(load().gn_graph_plan_blocked_cols(self._h))

    @property
    def blocked_gather_kernel(self) -> str:
        """The gather kernel the LDS-staged path launches for this plan: "staged", "direct" or "" (no such encoding)."""
        return ("", "staged", "direct")[int(load().gn_graph_plan_blocked_gather_kernel(self._h))]

    def blocked_waves(self) -> torch.Tensor:
        """[ranges, 16, 2] int64 on the CPU: (tiles, id-stream iterations) of every wave of every range's workgroup.
        (16 waves of 12 ints: the record gn_graph_plan_blocked_waves documents in include/gripnet_hip.h, kColWaves and
        kWaveInts of gcn_blocked.hip; a count that is no multiple of them raises here.)"""
        lib = load()
        n = int(lib.gn_graph_plan_blocked_waves(self._h, None, 0))
        cell = torch.zeros((n,), dtype=torch.int32)
        if n and lib.gn_graph_plan_blocked_waves(self._h, cell.data_ptr(), n) != n:
            raise GripNetHipError(GN_ERR_HIP, "gn_graph_plan_blocked_waves failed")
        if n % (16 * 12):
            raise GripNetHipError(GN_ERR_HIP, "gn_graph_plan_blocked_waves: {} ints are no whole number of 16 x 12 records".format(n))
        cell = cell.view(-1, 16, 12).long()
        return torch.stack([cell[:, :, 1] - cell[:, :, 0], cell[:, :, 3] - cell[:, :, 2]], dim=2)

    def blocked_ok(self, x: torch.Tensor, weight: torch.Tensor, bias, out: torch.Tensor) -> bool:
        """True when gn_graph_aggregate_f32(x, weight=W, bias, out) runs on the source-blocked kernels (the library's own
        answer: it sees the alignment of out and bias as well as of x)."""
        return bool(load().gn_graph_blocked_applicable(self._h, x.data_ptr(), ld(x), x.shape[1], weight.data_ptr(), weight.shape[1],
                                                       None if bias is None else bias.data_ptr(), out.data_ptr(), ld(out)))

    def transform_ok(self, fin: int, fout: int, x: torch.Tensor) -> bool:
        """True when gn_graph_aggregate_f32(weight=W) contracts with W in the gather's launch for this plan and input."""
        return (bool(load().gn_graph_transform_fusable(self._h, int(fin), int(fout))) and ld(x) % 4 == 0
                and x.data_ptr() % 16 == 0)

    @property
    def input_edges(self) -> int:
        return int(load().gn_graph_plan_input_edges(self._h))

    @property
    def nnz(self) -> int:
        return int(load().gn_graph_plan_nnz(self._h))

    def export(self):
        """(edge_index' [2,E'] int64, norm [E'] fp32) in the reference's order."""
        if self._export is None:
            n = self.nnz
            ei = torch.empty((2, n), dtype=torch.int64, device=self.device)
            nrm = torch.empty((n,), dtype=torch.float32, device=self.device)
            check(load().gn_graph_plan_export(self._h, ptr(ei), ptr(nrm), stream_ptr(self.device)))
            self._export = (ei, nrm)
        return self._export

    def __iter__(self):          # lets `edge_index, norm = conv.cached_result` keep working
        return iter(self.export())

    def _forward(self, entry, source, weight, bias, relu, out, side, planes, extra=()):
        """The forward launch `entry` over `source` (the gathered table's arguments: one table, or head and tail): the side
        copy's and the planes' descriptors, the planes' generation bumped once, the call under its tag."""
        sc = side_copy(side)
        pd = None
        if planes is not None:
            pd = planes[0].desc(planes[1], planes[2])
            planes[0].generation += 1
        _call(entry, self._h, *source, ptr(weight), 0 if weight is None else weight.shape[1], ptr(bias), int(bool(relu)),
              ptr(out), ld(out), _ref(sc), _ref(pd), *extra, stream_ptr(out.device), tag="{}[{}]".format(entry, self.kind))
        return out

    def aggregate(self, xw: torch.Tensor, bias, relu: bool, out: torch.Tensor, side=None, weight=None, planes=None, tail=None):
        """out = act(A_norm xw + b), or with `weight` act((A_norm xw) weight + b) (xw is then the layer input).
        `planes` = (SplitPlanes, col_main, col_side): the launch also leaves the bf16 split planes of its output and of
        its side copy.  `tail` = (W2 [16, 16], b2): every gathered row's last 16 columns enter the sum as
        relu(row[-16:] W2 + b2) (gn_graph_aggregate_tail_f32: 64 -> 16 features only, raises Unsupported otherwise)."""
        source = (ptr(xw), ld(xw), xw.shape[1])
        if tail is not None:
            return self._forward("gn_graph_aggregate_tail_f32", source, weight, bias, relu, out, side, planes,
                                 extra=(ptr(tail[0]), ptr(tail[1]), 1))
        return self._forward("gn_graph_aggregate_f32", source, weight, bias, relu, out, side, planes)

    def split_ok(self, head: torch.Tensor, tail: torch.Tensor, fout: int) -> bool:
        """True when `aggregate_split(head, tail, ...)` takes these operands (the library's own answer: widths, alignment,
        leading dimensions, environment switches).  Launches nothing."""
        return bool(load().gn_graph_split_applicable(self._h, head.data_ptr(), ld(head), head.shape[1], tail.data_ptr(), ld(tail),
                                                     head.shape[1] + tail.shape[1], int(fout)))

    def aggregate_split(self, head: torch.Tensor, tail: torch.Tensor, bias, relu: bool, out: torch.Tensor, weight: torch.Tensor,
                        side=None, planes=None):
        """`aggregate(cat([head, tail], 1), ..., weight=weight)` without the concatenation: a gathered row is read from the
        two tables where they lie (gn_graph_aggregate_split_f32; same bits; raises Unsupported for what it does not cover)."""
        source = (ptr(head), ld(head), head.shape[1], ptr(tail), ld(tail), head.shape[1] + tail.shape[1])
        return self._forward("gn_graph_aggregate_split_f32", source, weight, bias, relu, out, side, planes)

    def chain_ok(self, nxt: "GraphPlan", x: torch.Tensor, weight: torch.Tensor, bias, out: torch.Tensor, out_next: torch.Tensor) -> bool:
        """True when `aggregate_chain` / `nxt.gather_chained` can run this layer and the 16 -> 16 layer behind it (the
        library's own answer: plans, widths, alignment, environment switches)."""
        return bool(load().gn_graph_chain_applicable(self._h, nxt._h, x.data_ptr(), ld(x), x.shape[1], weight.data_ptr(),
                                                     weight.shape[1], None if bias is None else bias.data_ptr(),
                                                     out.data_ptr(), ld(out), out_next.data_ptr()))

    def aggregate_chain(self, nxt: "GraphPlan", x: torch.Tensor, weight: torch.Tensor, bias, relu: bool, out: torch.Tensor, side=None):
        """`aggregate(x, weight=weight)` on the LDS-staged kernels whose gather also fills `nxt`'s table with dis * out."""
        sc = side_copy(side)
        _call("gn_graph_aggregate_chain_f32", self._h, nxt._h, ptr(x), ld(x), x.shape[1], ptr(weight), weight.shape[1], ptr(bias),
              int(bool(relu)), ptr(out), ld(out), _ref(sc), stream_ptr(x.device))
        return out

    def gather_chained(self, out: torch.Tensor):
        """out[:, 0:16] = A_norm h, h the layer output the previous `aggregate_chain(nxt=self)` left in this plan's table."""
        _call("gn_graph_gather_chained_f32", self._h, ptr(out), ld(out), stream_ptr(out.device))
        return out

    def aggregate_bf16(self, xw: torch.Tensor, bias, relu: bool, out: torch.Tensor, side=None):
        """out = act(A_norm bf16(xw) + b): the gathered table is rounded to bf16 once and read at half the bytes;
        sums, bias, activation and `out` are fp32.  `xw` is the fp32 product (rounded here by gn_cast_bf16) or already the
        bf16 table (written by the product's own store, GN_GEMM_OUT_BF16: no extra pass)."""
        if xw.dtype == torch.bfloat16:
            table = xw
        else:
            table = torch.empty(xw.shape, dtype=torch.bfloat16, device=xw.device)
            _call("gn_cast_bf16", ptr(xw), ld(xw), ptr(table), ld(table), xw.shape[0], xw.shape[1], stream_ptr(xw.device))
        sc = side_copy(side)
        _call("gn_graph_aggregate_bf16", self._h, ptr(table), ld(table), xw.shape[1], ptr(bias), int(bool(relu)),
              ptr(out), ld(out), _ref(sc), stream_ptr(xw.device), tag="gn_graph_aggregate_bf16[{}]".format(self.kind))
        return out

    def build_transpose(self):
        """Add the source-major CSR (once; synchronises the stream): what a caller whose backward must not wait does up front."""
        if not getattr(self, "_has_t", False):
            with torch.cuda.device(self.device):
                check(load().gn_graph_plan_build_transpose(self._h, stream_ptr(self.device)))
            self._has_t = True
        return self

    def aggregate_t(self, g: torch.Tensor, out: torch.Tensor):
        """out[s] = sum over edges leaving s of coef * g[dst]: gradient of `aggregate` w.r.t. its table."""
        if not getattr(self, "_has_t", False):
            check(load().gn_graph_plan_build_transpose(self._h, stream_ptr(g.device)))
            self._has_t = True
        _call("gn_graph_aggregate_t_f32", self._h, ptr(g), ld(g), g.shape[1], ptr(out), ld(out), stream_ptr(g.device))
        return out


class RgcnPlan(Handle):
    """Owner of a gn_rgcn_plan handle (static multi-relational graph of one supervertex)."""
    _destroy = "gn_rgcn_plan_destroy"

    def __init__(self, edge_index, range_list, num_nodes, edge_lo=None, edge_hi=None, light=False, perm=None):
        """`light`: only what the general O(E) kernel reads (GN_RGCN_PLAN_LIGHT) - no host-built schedules: the plan of an edge
        list that will not be seen again.  `perm` ([E] int64, or None): the position of every listed edge in the caller's own
        list, where `edge_index` is a type-sorted copy of it (RGCNConv): a weighted call reads the caller's factors through it."""
        load()
        require_gpu(edge_index)
        ei, src, dst, e = edge_rows(edge_index)
        rl = torch.as_tensor(range_list).to("cpu", torch.int64).contiguous()   # tiny; host copy once
        if rl.dim() != 2 or rl.shape[1] != 2:
            raise ValueError("range_list must have shape [R, 2], got {}".format(tuple(rl.shape)))
        lo = 0 if edge_lo is None else int(edge_lo)
        hi = e if edge_hi is None else int(edge_hi)
        self._create("gn_rgcn_plan_create_ex", ei.device, src, dst, rl.data_ptr(), 1, rl.shape[0], e, int(num_nodes), lo, hi,
                     1 if light else 0)
        self.light = bool(light)
        self.device = ei.device
        self.num_nodes, self.num_relations, self.num_edges = int(num_nodes), int(rl.shape[0]), e
        self.edge_lo, self.edge_hi = lo, hi
        self._ws = None
        self._edge_index, self._range_list, self._wgrad = ei, rl, None
        self._deg = self._rev = self._pairs = None
        self._perm, self._has_pos = perm, False

    # What the backward pass needs of the graph, each part built on first use.  For a shard (edge_lo / edge_hi) the two plans
    # cover the shard's edges only - its share of the sums over edges - while the divisor is the in-degree over the FULL
    # graph, as in the forward.
    def in_degree(self):
        """[n] fp32: the mean's divisor of every destination, max(1, in-degree)."""
        if self._deg is None:
            ei = self._edge_index
            deg = torch.zeros(self.num_nodes, dtype=torch.float32, device=self.device)
            deg.index_add_(0, ei[1], torch.ones(e_count(ei), dtype=torch.float32, device=self.device))
            self._deg = deg.clamp_(min=1.0)
        return self._deg

    def reversed_plan(self):
        """The relational plan of the same edge positions with their endpoints swapped (dx is the layer on it)."""
        if self._rev is None:
            self._rev = RgcnPlan(self._edge_index.flip(0).contiguous(), self._range_list, self.num_nodes, self.edge_lo, self.edge_hi,
                                 perm=self._perm)           # (the same edge positions: the same permutation)
        return self._rev

    def pair_sums(self):
        """The plain-sum plan dst -> (relation, source) row: its aggregation of gm is Q [R * n, fout] of dW_r = X^T Q_r."""
        if self._pairs is None:
            ei, n, R = self._edge_index, self.num_nodes, self.num_relations
            sizes = (self._range_list[:, 1] - self._range_list[:, 0]).to(self.device)
            rel = torch.repeat_interleave(torch.arange(R, device=self.device), sizes)      # relation of every edge
            keyed = torch.stack([ei[1], rel * n + ei[0]])[:, self.edge_lo:self.edge_hi].contiguous()
            self._pairs = GraphPlan.plain_sum(keyed, n, R * n)
        return self._pairs

    def weight_grad_plan(self):
        """RelGradPlan of this layer's (shard's) edges, or None where the fused kernel does not apply (> 65534 nodes)."""
        if self._wgrad is None:
            try:
                self._wgrad = RelGradPlan(self.pair_sums(), self.num_nodes, self.num_relations)
            except Unsupported:
                self._wgrad = False
        return self._wgrad or None

    def general_weight_grad_supported(self, fin, fout) -> bool:
        return bool(load().gn_rgcn_weight_grad_supported(self._h, int(fin), int(fout)))

    def general_weight_grad(self, x, gm, supported=None, edge_weight=None):
        """dw [R, fin * fout] = sum over each relation's edges of x[src]^T gm[dst] on gn_rgcn_weight_grad_f32 (any number of
        nodes), or None where it does not cover the shapes (`supported`: that answer, from a caller that has asked).
        `edge_weight` ([E] fp32 in the order of the plan's own list): every edge's term times its factor."""
        fin, fout = x.shape[1], gm.shape[1]
        lib = load()
        if not (self.general_weight_grad_supported(fin, fout) if supported is None else supported):
            return None
        ei = self._edge_index
        dw = torch.empty((self.num_relations, fin * fout), dtype=torch.float32, device=x.device)
        need = int(lib.gn_rgcn_weight_grad_workspace_bytes(self._h, fin, fout))
        ws = torch.empty((need,), dtype=torch.uint8, device=x.device)
        base = ei.data_ptr()
        if edge_weight is None:
            _call("gn_rgcn_weight_grad_f32", self._h, base, base + 8 * self.num_edges, ptr(x), ld(x), fin, ptr(gm), ld(gm), fout, ptr(dw),
                  ptr(ws), need, stream_ptr(x.device))
        else:
            _call("gn_rgcn_weight_grad_weighted_f32", self._h, base, base + 8 * self.num_edges, ptr(edge_weight), ptr(x), ld(x), fin,
                  ptr(gm), ld(gm), fout, ptr(dw), ptr(ws), need, stream_ptr(x.device))
        if _recorder is not None:
            _recorder.keep.append(ei)
        return dw

    def _choice(self, x, fin, fout, bases, flags):
        """(kernel code, workspace bytes) of a forward with these shapes and flags: on `x` (its alignment picks the kernel),
        or, without one (a null x), on an aligned input - what gn_rgcn_forward_path and gn_rgcn_workspace_bytes answer."""
        need = C.c_size_t(0)
        at = (None, 0) if x is None else (x.data_ptr(), ld(x))
        code = int(load().gn_rgcn_forward_choice(self._h, at[0], at[1], fin, fout, bases, flags, C.byref(need)))
        return code, int(need.value)

    def _scratch(self, need):
        """The plan's scratch buffer, grown to `need` bytes."""
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=self.device)
        return self._ws

    def _workspace(self, x, fin, fout, bases, flags=0):
        need = self._choice(x, fin, fout, bases, flags)[1]
        return self._scratch(need), need

    @staticmethod
    def mode_flags(fast=False, path="auto"):
        """Arithmetic and kernel-choice bits of gn_rgcn_forward_f32."""
        return (GN_RGCN_ARITH_FAST if fast else 0) | (RGCN_PATHS[path] << GN_RGCN_PATH_SHIFT)

    def path(self, fin, fout, bases, fast=False, path="auto", x=None):
        """Name of the kernel a forward with these shapes and flags takes (on `x` when given, else on an aligned input)."""
        code = self._choice(x, fin, fout, bases, self.mode_flags(fast, path))[0]
        return RGCN_PATH_NAMES.get(code, "?")

    def weighted_supported(self, fin, fout, bases) -> bool:
        return bool(load().gn_rgcn_weighted_supported(self._h, int(fin), int(fout), int(bases)))

    def build_positions(self):
        """The position list of the weighted calls (4 bytes per edge, built on the device; it synchronises the stream once)."""
        if not self._has_pos:
            ei = self._edge_index
            with torch.cuda.device(self.device):
                check(load().gn_rgcn_plan_build_positions(self._h, ei.data_ptr() + 8 * self.num_edges, ptr(self._perm), stream_ptr(self.device)))
            self._has_pos = True
        return self

    def forward_weighted(self, x, basis, att, root, bias, relu, out, edge_weight, partial=False):
        """The sum (or, `partial`, the bare edge sums) with the factor `edge_weight[e]` on every message: [E] fp32 in the
        caller's order (the order `perm` maps to), read through the position list.  General kernel only."""
        fin, fout, bases = x.shape[1], basis.shape[2], basis.shape[0]
        self.build_positions()
        need = int(load().gn_rgcn_weighted_workspace_bytes(self._h, fin, fout, bases))
        _call("gn_rgcn_forward_weighted_f32", self._h, ptr(x), ld(x), fin, ptr(basis), ptr(att), bases, ptr(root), ptr(bias), fout,
              int(bool(relu)), GN_RGCN_PARTIAL if partial else GN_RGCN_SUM, ptr(edge_weight), ptr(out), ld(out), ptr(self._scratch(need)), need,
              stream_ptr(x.device))
        return out

    def forward(self, x, basis, att, root, bias, relu, out, partial=False, side=None, fast=False, path="auto", x_planes=None,
                basis_transposed=False, sum_edges=False):
        """`x_planes`: SplitPlanes of x left by its producer (the destination-major kernel then skips its own split of x;
        the other kernels ignore them).  `basis_transposed`: `basis` is [bases, out, in] (the forward's parameter seen from
        the reversed layer of its backward; destination-major kernel only: GN_RGCN_BASIS_TRANSPOSED)."""
        mode = self.mode_flags(fast, path) | (GN_RGCN_SUM if sum_edges else 0)    # (sum_edges: GN_RGCN_SUM - no divisor, root may be None)
        fout = basis.shape[1] if basis_transposed else basis.shape[2]
        ws, need = self._workspace(x, x.shape[1], fout, basis.shape[0], mode)
        sc = side_copy(side)
        flags = (GN_RGCN_PARTIAL if partial else 0) | mode | (GN_RGCN_BASIS_TRANSPOSED if basis_transposed else 0)
        _call("gn_rgcn_forward_f32", self._h, ptr(x), ld(x), x.shape[1], ptr(basis), ptr(att), basis.shape[0],
              ptr(root), ptr(bias), fout, int(bool(relu)), flags,
              ptr(out), ld(out), _ref(sc), None if x_planes is None else x_planes.buf.data_ptr(), ptr(ws), need,
              stream_ptr(x.device))
        return out

    def finalize(self, summed, x, root, bias, relu, out, side=None):
        sc = side_copy(side)
        _call("gn_rgcn_finalize_f32", self._h, ptr(summed), ld(summed), ptr(x), ld(x), x.shape[1], ptr(root),
              ptr(bias), root.shape[1], int(bool(relu)), ptr(out), ld(out), _ref(sc), stream_ptr(x.device))
        return out


def error_flag(device) -> torch.Tensor:
    """Per-device int32 word the decoder kernels OR index-range errors into (checked lazily)."""
    return zeroed_once(device, "errors", 1, torch.int32)


def raise_if_index_errors(device=None):
    """Synchronising check of the error word; raises IndexError like the reference's advanced indexing would
    (gripnet/decoder.py:20; for class ids, the loss line score[range(n), classes] of the NC drivers)."""
    for (kind, index, what), flag in list(_zeroed.items()):
        if what != "errors" or (device is not None and (device.type, device.index) != (kind, index)):
            continue
        bits = int(flag.item())
        if bits != 0:
            flag.zero_()
            if bits & 4:
                raise RuntimeError("one-shot exchange: a peer's partial sums did not arrive within the timeout")
            if bits & 2:
                raise RuntimeError("negative sampler: a relation's positive pairs leave no pair to draw "
                                   "(or a KGE candidate row's known partners no entity)")
            found = []
            if bits & 1:
                found.append("DistMult decoder saw an edge endpoint or relation id outside its table (or a KGE scorer a head, tail or relation id)")
            if bits & 8:
                found.append("class metrics saw a class id outside [0, num_class) (true or predicted)")
            raise IndexError("; ".join(found))


def distmult(z, u_v, edge_type, weight, sigmoid, out):
    ei, u, v, e = edge_rows(u_v)
    et = i64_vec(edge_type)
    if et.numel() != e:
        raise ValueError("edge_type has {} entries for {} edges".format(et.numel(), e))
    _call("gn_distmult_forward_f32", ptr(z), ld(z), z.shape[0], z.shape[1], u, v, ptr(et), ptr(weight),
          ld(weight), weight.shape[0], e, int(bool(sigmoid)), ptr(out),
          ptr(error_flag(z.device)), stream_ptr(z.device))
    return out


_ids16 = VersionedCache(4)         # edge_type tensor -> its int16 copy


def relation_ids16(et):
    """The relation ids of a (static) edge_type tensor as 16-bit values, narrowed once per tensor and version."""
    if et.dtype == torch.int16:                         # (`to` would return `et` itself: a value that keeps its own key alive)
        return et
    r16 = _ids16.get(et)
    return _ids16.put(et, et.to(torch.int16)) if r16 is MISS else r16


def packed_pairs(edge_index):
    """The (uint32 words, as int32) that NegativeSampler.sample left next to an edge list, or None (another list, or
    the list was modified since)."""
    tag = getattr(edge_index, "_gn_packed", None)
    if tag is None or tag[1] != edge_index._version:
        return None
    return tag[0]


def distmult_packed(z, packed, edge_type, weight, sigmoid, out):
    e = int(packed.numel())
    if edge_type.numel() != e:
        raise ValueError("edge_type has {} entries for {} edges".format(edge_type.numel(), e))
    r16 = relation_ids16(edge_type)
    _call("gn_distmult_packed_forward_f32", ptr(z), ld(z), z.shape[0], z.shape[1], ptr(packed), ptr(r16), ptr(weight),
          ld(weight), weight.shape[0], e, int(bool(sigmoid)), ptr(out), ptr(error_flag(z.device)), stream_ptr(z.device))
    return out


def distmult_any(z, u_v, edge_type, weight, sigmoid, out):
    """The plan-less decoder: on the packed pairs a NegativeSampler left with `u_v` when there are any (and ids fit 16
    bits), else on the raw int64 triples."""
    packed = packed_pairs(u_v)
    if packed is not None and z.shape[0] <= 65535 and weight.shape[0] <= 32767:
        try:
            return distmult_packed(z, packed, edge_type, weight, sigmoid, out)
        except Unsupported:                     # node table too large for the LDS: the general kernels
            pass
    return distmult(z, u_v, edge_type, weight, sigmoid, out)


def distmult_forward(z, u_v, edge_type, weight, sigmoid, out, plan=None):
    """The decoder's forward ladder: the DistMultPlan of a static list (the positives: same bits, fewer bytes) when there is
    one and it takes this call, else `distmult_any`.  Returns (out, served): served is False when `plan` did not carry the
    call (none given, or it refused: node table too large for the LDS).  A refusal can depend on this call's `z`, so the
    plan is not marked here: a caller that wants to stop asking does that itself."""
    if plan is not None:
        try:
            return plan.forward(z, weight, sigmoid, out), True
        except Unsupported:
            pass
    return distmult_any(z, u_v, edge_type, weight, sigmoid, out), False


class DistMultPlan(Handle):
    """Owner of a gn_distmult_plan handle: one static (edge_index, edge_type) list, validated, packed and ordered
    for the LDS-resident decoder kernel (the positive edges a training loop scores every epoch)."""
    _destroy = "gn_distmult_plan_destroy"

    def __init__(self, u_v, edge_type, num_nodes, num_relations, num_features=0):
        """`num_features` (the decoder's in_dim; 0: unknown) lets the plan add the row-class encoding: whole rows of a
        class of nodes in LDS, one table fill per launch (k_distmult_class)."""
        load()
        require_gpu(u_v, edge_type)
        ei, u, v, e = edge_rows(u_v)
        et = i64_vec(edge_type)
        if et.numel() != e:
            raise ValueError("edge_type has {} entries for {} edges".format(et.numel(), e))
        self._create("gn_distmult_plan_create", ei.device, u, v, ptr(et), e, int(num_nodes), int(num_relations), int(num_features))
        self.device, self.num_edges = ei.device, e
        self.num_nodes, self.num_relations = int(num_nodes), int(num_relations)
        self._bwd = None                     # None: not asked for yet; False: the library refused it; else DistMultBwdPlan

    def backward_plan(self, u_v, edge_type):
        """The DistMultBwdPlan of my list (`u_v`, `edge_type`: the tensors I was built from), or None where the library
        refuses one (tables too large for the LDS path): built at the first request - the sort happens once per static
        edge list, not once per step - and kept with me."""
        if self._bwd is None:
            try:
                self._bwd = DistMultBwdPlan(u_v, edge_type, self.num_nodes, self.num_relations)
            except Unsupported:
                self._bwd = False
        return self._bwd or None

    def forward(self, z, weight, sigmoid, out):
        _call("gn_distmult_plan_forward_f32", self._h, ptr(z), ld(z), z.shape[1], ptr(weight), ld(weight),
              int(bool(sigmoid)), ptr(out), stream_ptr(z.device))
        return out

    def forward_cols(self, z, num_features, col_lo, col_hi, weight, sigmoid, out):
        """Feature columns [col_lo, col_hi) of the scores (z may hold the first col_hi columns only); the launch with
        col_lo = 0 starts the sums in `out`, the one with col_hi = num_features finishes them."""
        _call("gn_distmult_plan_forward_cols_f32", self._h, ptr(z), ld(z), int(num_features), int(col_lo), int(col_hi),
              ptr(weight), ld(weight), int(bool(sigmoid)), ptr(out), stream_ptr(z.device))
        return out


class RelGradPlan(Handle):
    """Owner of a gn_rel_grad_plan handle: the edge-dependent part of the relational layer's weight gradient
    (dW_r = X^T Q_r in one launch), built from the layer's (relation, source)-major sum plan."""
    _destroy = "gn_rel_grad_plan_destroy"

    def __init__(self, sums: "GraphPlan", num_nodes, num_relations):
        self._create("gn_rel_grad_plan_create", sums.device, sums._h, int(num_nodes), int(num_relations))
        self.device, self.num_relations = sums.device, int(num_relations)

    def supported(self, fin, fout) -> bool:
        return bool(load().gn_rel_weight_grad_supported(self._h, int(fin), int(fout)))

    def weight_grad(self, x, gm, out=None):
        """dw [R, fin * fout]: dw[r] = sum over the edges e of relation r of x[src_e]^T gm[dst_e]."""
        fin, fout = x.shape[1], gm.shape[1]
        if out is None:
            out = torch.empty((self.num_relations, fin * fout), dtype=torch.float32, device=x.device)
        _call("gn_rel_weight_grad_f32", self._h, ptr(x), ld(x), fin, ptr(gm), ld(gm), fout, ptr(out), stream_ptr(x.device))
        return out


class DistMultBwdPlan(Handle):
    """Owner of a gn_distmult_bwd_plan handle: the gradient-independent part of the decoder's backward pass for one
    static (edge_index, edge_type) list."""
    _destroy = "gn_distmult_bwd_plan_destroy"

    def __init__(self, u_v, edge_type, num_nodes, num_relations):
        load()
        require_gpu(u_v, edge_type)
        ei, u, v, e = edge_rows(u_v)
        et = i64_vec(edge_type)
        self._create("gn_distmult_bwd_plan_create", ei.device, u, v, ptr(et), e, int(num_nodes), int(num_relations))
        self.device, self.num_edges = ei.device, e
        self.num_nodes, self.num_relations = int(num_nodes), int(num_relations)

    def backward(self, z, weight, grad_logit, dz, dd, probs=None, loss=None):
        """`loss` (a LinkLossGrad; then grad_logit is None and probs the forward's probabilities): the scores feed the link loss
        directly - its derivative is computed where the records are built (gn_distmult_backward_loss_planned_f32)."""
        n_grad = probs.numel() if loss is not None else grad_logit.numel()
        if n_grad != self.num_edges:
            raise ValueError("the plan was built from {} edges, got {} gradients".format(self.num_edges, n_grad))
        need = int(load().gn_distmult_bwd_plan_workspace_bytes(self._h, z.shape[1]))
        ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=z.device)
        if loss is not None:
            _call("gn_distmult_backward_loss_planned_f32", self._h, ptr(z), ld(z), z.shape[1], ptr(weight), ld(weight),
                  loss.ref(), ptr(probs), ptr(dz), ld(dz), ptr(dd), ld(dd), ptr(ws), need, stream_ptr(z.device))
            return dz, dd
        _call("gn_distmult_backward_planned_f32", self._h, ptr(z), ld(z), z.shape[1], ptr(weight), ld(weight),
              ptr(grad_logit), ptr(probs), ptr(dz), ld(dz), ptr(dd), ld(dd), ptr(ws), need, stream_ptr(z.device))
        return dz, dd


_type_offsets = VersionedCache(4)           # (edge_type tensor, relations) -> offsets + task list, or None: not sorted


_batch_tls = threading.local()      # the open batch of THIS thread: the library's queue is thread_local too (autograd runs a
                                    # device's backward on its own thread; two GPUs in one process must not see each other's batch)


class dense_batch:
    """``with dense_batch(device):`` - the deep-and-narrow `gemm` calls and the one-launch `xtg` calls inside leave as ONE
    launch at the end of the block (gn_dense_batch_begin / _end); they must not depend on each other.  The operands of
    every `gemm` / `xtg` call inside are kept alive until the batch has been launched (a temporary freed in between could
    be handed out again and overwritten before the queued product reads it)."""

    def __init__(self, device):
        self.device, self.keep = device, []

    def __enter__(self):
        self.off = os.environ.get("GN_DENSE_BATCH") == "0"     # (development switch: every product launches on its own)
        if self.off:
            return self
        _call("gn_dense_batch_begin")
        _batch_tls.open = self
        return self

    def __exit__(self, *exc):
        if self.off:
            return False
        _batch_tls.open = None
        try:
            with torch.cuda.device(self.device):
                _call("gn_dense_batch_end", stream_ptr(self.device))
        finally:
            self.keep = []
        return False


def type_offsets(et, num_relations):
    """[R + 1] int32 offsets of the relations in a non-decreasing edge_type tensor, or None if it is not sorted.  One
    device reduction and host read per tensor (and version): the reference passes the same `train_et` with the
    positive and the negative edges of every epoch."""
    off = _type_offsets.get(et, num_relations)
    if off is not MISS:
        return off
    off = None
    if et.numel() < 2 or bool((et[1:] >= et[:-1]).all()):
        bounds = torch.arange(num_relations + 1, device=et.device, dtype=et.dtype)
        first = torch.searchsorted(et.contiguous(), bounds).to(torch.int32)
        # the offsets and, behind them, the task list of the decoder gradient's relation-major pass (GN_DM_TYPE_TASKS)
        lib = load()
        need = int(lib.gn_distmult_type_tasks_bytes(num_relations, et.numel()))
        off = torch.empty((need // 4,), dtype=torch.int32, device=et.device)
        with torch.cuda.device(et.device):
            _call("gn_distmult_type_tasks", ptr(first), num_relations, et.numel(), ptr(off), need, stream_ptr(et.device))
    return _type_offsets.put(et, off, num_relations)


class LinkLossGrad:
    """gn_link_loss_grad: where the decoder's backward gets d loss / d probability from when its scores feed the link loss of
    GripNet-pose.py:140-142 directly (upstream: the loss's one upstream gradient, a device scalar, or None for 1)."""

    class _S(C.Structure):
        _fields_ = [("upstream", C.c_void_p), ("eps", C.c_float), ("negative", C.c_int)]

    def __init__(self, upstream, eps, negative):
        self.upstream = upstream                               # (kept alive with the call's operands)
        self._s = LinkLossGrad._S(None if upstream is None else upstream.data_ptr(), float(eps), 1 if negative else 0)

    def ref(self):
        if _recorder is not None:
            _recorder.keep.append(self)
        return C.addressof(self._s)


def distmult_backward_loss_packed(z, u_v, edge_type, weight, probs, dz, dd, loss, dz_add=None, dd_add=None):
    """The loss-fed backward on the sampler's packed pairs (gn_distmult_backward_loss_packed_f32), or False where that path
    does not apply (no packed pairs, unsorted types, tables beyond the counting-sort path): the caller takes the two-step path.
    `dz_add` / `dd_add`: the other list's gradients of z and D, added where this call stores its sums (they may be dz / dd)."""
    e = e_count(u_v)
    offsets = type_offsets(edge_type, weight.shape[0])
    packed = packed_pairs(u_v)
    if packed is None or offsets is None or z.shape[0] > 65535 or weight.shape[0] > 32767:
        return False
    need = int(load().gn_distmult_backward_workspace_bytes(z.shape[0], z.shape[1], weight.shape[0], e))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=z.device)
    try:
        _call("gn_distmult_backward_loss_packed_f32", ptr(z), ld(z), z.shape[0], z.shape[1], ptr(packed), ptr(relation_ids16(edge_type)),
              ptr(weight), ld(weight), weight.shape[0], e, loss.ref(), ptr(probs), ptr(dz), ld(dz), ptr(dd), ld(dd),
              GN_DM_TYPES_SORTED | GN_DM_TYPE_TASKS, ptr(offsets), ptr(dz_add), 0 if dz_add is None else ld(dz_add),
              ptr(dd_add), 0 if dd_add is None else ld(dd_add), ptr(ws), need, stream_ptr(z.device))
    except Unsupported:
        return False
    return True


def distmult_backward(z, u_v, edge_type, weight, grad_logit, dz, dd, probs=None):
    """`probs`: the sigmoid scores of the forward; grad_logit is then the gradient with respect to them."""
    ei, u, v, e = edge_rows(u_v)
    et = i64_vec(edge_type)
    offsets = type_offsets(edge_type, weight.shape[0])
    flags = (GN_DM_TYPES_SORTED | GN_DM_TYPE_TASKS) if offsets is not None else 0
    need = int(load().gn_distmult_backward_workspace_bytes(z.shape[0], z.shape[1], weight.shape[0], e))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=z.device)
    packed = packed_pairs(u_v)
    if packed is not None and offsets is not None and z.shape[0] <= 65535 and weight.shape[0] <= 32767:
        # the sampler's 32-bit pairs + the static edge_type's 16-bit ids: 6 instead of 24 bytes per edge and sort pass
        try:
            _call("gn_distmult_backward_packed_f32", ptr(z), ld(z), z.shape[0], z.shape[1], ptr(packed), ptr(relation_ids16(edge_type)),
                  ptr(weight), ld(weight), weight.shape[0], e, ptr(grad_logit), ptr(dz), ld(dz), ptr(dd), ld(dd), flags, ptr(probs),
                  ptr(offsets), ptr(ws), need, stream_ptr(z.device))
            return dz, dd
        except Unsupported:                     # tables too large for the counting-sort path: the int64 call
            pass
    _call("gn_distmult_backward_ex_f32", ptr(z), ld(z), z.shape[0], z.shape[1], u, v, ptr(et), ptr(weight), ld(weight),
          weight.shape[0], e, ptr(grad_logit), ptr(dz), ld(dz), ptr(dd), ld(dd), flags, ptr(probs), ptr(offsets), ptr(ws),
          need, stream_ptr(z.device))
    return dz, dd


def distmult_backward_planned(plan, z, u_v, edge_type, weight, grad_logit, dz, dd, probs=None, loss=None):
    """The decoder's backward ladder for a list that may have a static `plan` (a DistMultPlan or None): the launch on the
    plan's backward plan; where there is none or it refuses (unaligned rows), the plan-less entry points
    (`distmult_backward`).  With `loss` (a LinkLossGrad; grad_logit is None) only the loss-fed planned launch is tried.
    Returns False when nothing was launched (loss-fed and no plan took it: the caller takes the two-step path)."""
    bwd = None if plan is None else plan.backward_plan(u_v, edge_type)
    if bwd is not None:
        try:
            bwd.backward(z, weight, grad_logit, dz, dd, probs, loss=loss)
            return True
        except Unsupported:
            pass
    if loss is not None:
        return False
    distmult_backward(z, u_v, edge_type, weight, grad_logit, dz, dd, probs=probs)
    return True


KGE_MODELS = {"TransE": 0, "DistMult": 1, "ComplEx": 2, "RotatE": 3}          # GN_KGE_* of include/gripnet_hip.h


def _kge_hidden(model, ent, rel):
    """(GN_KGE_* id, hidden size) of a pair of tables, their widths checked against each other."""
    m = KGE_MODELS[model]
    h = rel.shape[1] // 2 if model == "ComplEx" else rel.shape[1]
    de = 2 * h if model in ("ComplEx", "RotatE") else h
    if ent.shape[1] != de or (model == "ComplEx" and rel.shape[1] != 2 * h):
        raise ValueError("{}: entity rows of {} and relation rows of {} columns do not belong together".format(
            model, ent.shape[1], rel.shape[1]))
    return m, h


def _kge_operands(model, ent, rel, sample, et):
    """(hidden size, kept-alive index tensor, head pointer, tail pointer, E, edge_type) of a KGE call, shapes checked."""
    m, h = _kge_hidden(model, ent, rel)
    idx, head, tail, e = edge_rows(sample)
    types = i64_vec(et)
    if types.numel() != e:
        raise ValueError("edge_type has {} entries for {} triples".format(types.numel(), e))
    return m, h, idx, head, tail, e, types


_sorted_types = VersionedCache(4)          # edge_type tensor -> whether it is non-decreasing


def _non_decreasing(et):
    """One device reduction and host read per tensor (and version): the reference scores its static `train_et` every step."""
    known = _sorted_types.get(et)
    if known is MISS:
        known = _sorted_types.put(et, bool((et[1:] >= et[:-1]).all()))
    return known


def kge_forward(model, ent, rel, sample, et, gamma, divisor, log_sigmoid, out, raw=None):
    """gn_kge_forward_f32: the scores of `sample` [2, E] under `model` into `out` (with `log_sigmoid`: their log-sigmoid,
    the raw scores into `raw`).  Ids outside the tables: NaN and the device's error flag (raise_if_index_errors)."""
    m, h, idx, head, tail, e, types = _kge_operands(model, ent, rel, sample, et)
    need = int(load().gn_kge_forward_workspace_bytes(m, rel.shape[0], h))
    ws = torch.empty((need,), dtype=torch.uint8, device=ent.device) if need else None
    _call("gn_kge_forward_f32", m, ptr(ent), ld(ent), ent.shape[0], ptr(rel), ld(rel), rel.shape[0], h, head, tail, ptr(types), e,
          float(gamma), float(divisor), int(bool(log_sigmoid)), ptr(out), ptr(raw), ptr(error_flag(ent.device)), ptr(ws), need,
          stream_ptr(ent.device))
    return out


def kge_backward(model, ent, rel, sample, et, divisor, grad_out, raw, d_ent, d_rel, types_sorted=None):
    """gn_kge_backward_f32: d_ent / d_rel (overwritten) from the gradient of the forward's output; `raw`: the raw scores
    when that output was the log-sigmoid.  `types_sorted` None: looked up (once per edge_type tensor and version)."""
    m, h, idx, head, tail, e, types = _kge_operands(model, ent, rel, sample, et)
    if types_sorted is None:
        types_sorted = e < 2 or _non_decreasing(et)
    need = int(load().gn_kge_backward_workspace_bytes(m, ent.shape[0], rel.shape[0], h, e))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=ent.device)
    _call("gn_kge_backward_f32", m, ptr(ent), ld(ent), ent.shape[0], ptr(rel), ld(rel), rel.shape[0], h, head, tail, ptr(types), e,
          float(divisor), ptr(grad_out), ptr(raw), ptr(d_ent), ld(d_ent), ptr(d_rel), ld(d_rel),
          GN_DM_TYPES_SORTED if types_sorted else 0, ptr(ws), need, stream_ptr(ent.device))
    return d_ent, d_rel


def _kge_batch_operands(model, ent, rel, fixed, et, cand, side):
    """(model id, hidden size, side id, fixed, edge_type, candidates as the kernels read them, B, K) of a candidate-block
    call, shapes checked.  `cand` [B, K] int64 keeps a row stride above K (a column slice of a wider matrix); any other
    layout is copied."""
    m, h = _kge_hidden(model, ent, rel)
    if side not in KGE_SIDES:
        raise ValueError("side must be 'tail' or 'head', got {!r}".format(side))
    fixed, types = i64_vec(fixed), i64_vec(et)
    if fixed.dim() != 1 or types.dim() != 1 or types.numel() != fixed.numel():
        raise ValueError("fixed entities {} and edge_type {} must be two vectors of one length".format(
            tuple(fixed.shape), tuple(types.shape)))
    b = int(fixed.numel())
    if cand.dtype != torch.int64:
        raise TypeError("indices must be int64 (torch.long), got {}".format(cand.dtype))
    if cand.dim() != 2 or cand.shape[0] != b:
        raise ValueError("candidates must have shape [{}, K], got {}".format(b, tuple(cand.shape)))
    k = int(cand.shape[1])
    if (k > 1 and cand.stride(1) != 1) or (b > 1 and cand.stride(0) < k):
        cand = cand.contiguous()
    return m, h, KGE_SIDES[side], fixed, types, cand, b, k


def kge_batch_forward(model, ent, rel, fixed, et, cand, side, gamma, divisor, log_sigmoid, out, raw=None):
    """gn_kge_batch_forward_f32: out[b, k] (fp32 [B, K], contiguous) = the score of (fixed[b], et[b], cand[b, k]) for
    `side` "tail", of (cand[b, k], et[b], fixed[b]) for "head" (with `log_sigmoid`: its log-sigmoid, the raw scores into
    `raw`) - the bits of kge_forward on the expanded list.  Ids outside the tables: NaN (a bad fixed entity or relation:
    the whole row) and the device's error flag (raise_if_index_errors)."""
    m, h, sd, fixed, types, cand, b, k = _kge_batch_operands(model, ent, rel, fixed, et, cand, side)
    need = int(load().gn_kge_batch_forward_workspace_bytes(m, rel.shape[0], h))
    ws = torch.empty((need,), dtype=torch.uint8, device=ent.device) if need else None
    _call("gn_kge_batch_forward_f32", m, ptr(ent), ld(ent), ent.shape[0], ptr(rel), ld(rel), rel.shape[0], h, ptr(fixed), ptr(types),
          ptr(cand), ld(cand), b, k, sd, float(gamma), float(divisor), int(bool(log_sigmoid)), ptr(out), ptr(raw),
          ptr(error_flag(ent.device)), ptr(ws), need, stream_ptr(ent.device))
    return out


def kge_batch_backward(model, ent, rel, fixed, et, cand, side, divisor, grad_out, raw, d_ent, d_rel, types_sorted=None):
    """gn_kge_batch_backward_f32: d_ent / d_rel (overwritten) from the gradient [B, K] of kge_batch_forward's output; `raw`:
    the raw scores when that output was the log-sigmoid.  `types_sorted` None: looked up (once per edge_type tensor and
    version)."""
    m, h, sd, fixed, types, cand, b, k = _kge_batch_operands(model, ent, rel, fixed, et, cand, side)
    if types_sorted is None:
        types_sorted = b < 2 or _non_decreasing(et)
    need = int(load().gn_kge_batch_backward_workspace_bytes(m, ent.shape[0], rel.shape[0], h, b, k))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=ent.device)
    _call("gn_kge_batch_backward_f32", m, ptr(ent), ld(ent), ent.shape[0], ptr(rel), ld(rel), rel.shape[0], h, ptr(fixed), ptr(types),
          ptr(cand), ld(cand), b, k, sd, float(divisor), ptr(grad_out), ptr(raw), ptr(d_ent), ld(d_ent), ptr(d_rel), ld(d_rel),
          GN_DM_TYPES_SORTED if types_sorted else 0, ptr(ws), need, stream_ptr(ent.device))
    return d_ent, d_rel


def _kge_shared_operands(model, ent, rel, fixed, et, cand, side):
    """(model id, hidden size, side id, fixed, edge_type, candidate lists as the kernels read them, B, G, K) of a
    shared-list call, shapes checked: `cand` [G, K] int64 with 1 <= G <= B and B % G == 0 (a row stride above K is kept,
    any other layout is copied); entity rows of at most KGE_SHARED_MAX_ROW floats."""
    m, h = _kge_hidden(model, ent, rel)
    if side not in KGE_SIDES:
        raise ValueError("side must be 'tail' or 'head', got {!r}".format(side))
    if ent.shape[1] > KGE_SHARED_MAX_ROW:
        raise ValueError("{}: the shared-list kernels take entity rows of at most {} floats (hidden_dim <= {}), got {}".format(
            model, KGE_SHARED_MAX_ROW, KGE_SHARED_MAX_ROW * h // ent.shape[1], ent.shape[1]))
    fixed, types = i64_vec(fixed), i64_vec(et)
    if fixed.dim() != 1 or types.dim() != 1 or types.numel() != fixed.numel():
        raise ValueError("fixed entities {} and edge_type {} must be two vectors of one length".format(
            tuple(fixed.shape), tuple(types.shape)))
    b = int(fixed.numel())
    if cand.dtype != torch.int64:
        raise TypeError("indices must be int64 (torch.long), got {}".format(cand.dtype))
    if cand.dim() != 2 or not 1 <= cand.shape[0] <= max(b, 1) or b % cand.shape[0] != 0:
        raise ValueError("shared candidates must have shape [G, K] with G dividing the {} positives, got {}".format(
            b, tuple(cand.shape)))
    g, k = int(cand.shape[0]), int(cand.shape[1])
    if (k > 1 and cand.stride(1) != 1) or (g > 1 and cand.stride(0) < k):
        cand = cand.contiguous()
    return m, h, KGE_SIDES[side], fixed, types, cand, b, g, k


def kge_shared_forward(model, ent, rel, fixed, et, cand, side, gamma, divisor, log_sigmoid, out, raw=None):
    """gn_kge_shared_forward_f32: out[b, k] (fp32 [B, K], contiguous) = the score of (fixed[b], et[b], cand[g, k]) for
    `side` "tail", of (cand[g, k], et[b], fixed[b]) for "head", g = b // (B // G) (with `log_sigmoid`: its log-sigmoid,
    the raw scores into `raw`).  Ids outside the tables: NaN (a bad fixed entity or relation: the whole row; a bad
    candidate: its column of its chunk) and the device's error flag (raise_if_index_errors)."""
    m, h, sd, fixed, types, cand, b, g, k = _kge_shared_operands(model, ent, rel, fixed, et, cand, side)
    need = int(load().gn_kge_shared_forward_workspace_bytes(m, rel.shape[0], h))
    ws = torch.empty((need,), dtype=torch.uint8, device=ent.device) if need else None
    _call("gn_kge_shared_forward_f32", m, ptr(ent), ld(ent), ent.shape[0], ptr(rel), ld(rel), rel.shape[0], h, ptr(fixed), ptr(types),
          ptr(cand), ld(cand), b, g, k, sd, float(gamma), float(divisor), int(bool(log_sigmoid)), ptr(out), ptr(raw),
          ptr(error_flag(ent.device)), ptr(ws), need, stream_ptr(ent.device))
    return out


def kge_shared_backward(model, ent, rel, fixed, et, cand, side, divisor, grad_out, raw, d_ent, d_rel, types_sorted=None):
    """gn_kge_shared_backward_f32: d_ent / d_rel (overwritten) from the gradient [B, K] of kge_shared_forward's output;
    `raw`: the raw scores when that output was the log-sigmoid.  `types_sorted` None: looked up (once per edge_type tensor
    and version)."""
    m, h, sd, fixed, types, cand, b, g, k = _kge_shared_operands(model, ent, rel, fixed, et, cand, side)
    if types_sorted is None:
        types_sorted = b < 2 or _non_decreasing(et)
    need = int(load().gn_kge_shared_backward_workspace_bytes(m, ent.shape[0], rel.shape[0], h, b, g, k))
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=ent.device)
    _call("gn_kge_shared_backward_f32", m, ptr(ent), ld(ent), ent.shape[0], ptr(rel), ld(rel), rel.shape[0], h, ptr(fixed), ptr(types),
          ptr(cand), ld(cand), b, g, k, sd, float(divisor), ptr(grad_out), ptr(raw), ptr(d_ent), ld(d_ent), ptr(d_rel), ld(d_rel),
          GN_DM_TYPES_SORTED if types_sorted else 0, ptr(ws), need, stream_ptr(ent.device))
    return d_ent, d_rel


def kge_ns_block(pos, neg):
    """(B, K) of a score block of the negative-sampling loss: pos fp32 [B] contiguous, neg fp32 [B, K] with unit inner
    stride and a row stride of at least K (what KgeNegativeSamplingLossFn hands on)."""
    b, k = int(neg.shape[0]), int(neg.shape[1])
    if b < 1 or k < 1:
        raise ValueError("the loss needs at least one positive and one negative each, got {}".format(tuple(neg.shape)))
    return b, k


def kge_ns_loss_forward(pos, neg, weight=None, temperature=None):
    """(loss 0-d, row_stats [B, 2], scale [1]) of gn_kge_ns_loss_forward_f32; its per-device scratch is zeroed once (the
    kernel leaves it ready for the next launch).  `temperature` None: the negatives of a row are averaged."""
    b, k = kge_ns_block(pos, neg)
    dev = pos.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    stats = torch.empty((b, 2), dtype=torch.float32, device=dev)
    scale = torch.empty((1,), dtype=torch.float32, device=dev)
    ws = zeroed_once(dev, "kge ns loss", lambda: load().gn_kge_ns_loss_workspace_bytes(b))
    _call("gn_kge_ns_loss_forward_f32", ptr(pos), ptr(neg), ld(neg), b, k, ptr(weight), int(temperature is not None),
          float(temperature or 0.0), ptr(loss), ptr(stats), ptr(scale), ptr(ws), ws.numel(), stream_ptr(dev))
    return loss, stats, scale


def kge_ns_loss_backward(pos, neg, weight, temperature, stats, scale, g, d_pos=None, d_neg=None):
    """(d_pos [B], d_neg [B, K]) of gn_kge_ns_loss_backward_f32 from what the forward left in `stats` and `scale`; `g`: the
    upstream gradient, a contiguous fp32 scalar on the device, or None for 1."""
    b, k = kge_ns_block(pos, neg)
    d_pos = torch.empty((b,), dtype=torch.float32, device=pos.device) if d_pos is None else d_pos
    d_neg = torch.empty((b, k), dtype=torch.float32, device=pos.device) if d_neg is None else d_neg
    _call("gn_kge_ns_loss_backward_f32", ptr(pos), ptr(neg), ld(neg), b, k, ptr(weight), int(temperature is not None),
          float(temperature or 0.0), ptr(stats), ptr(scale), ptr(g), ptr(d_pos), ptr(d_neg), ld(d_neg), stream_ptr(pos.device))
    return d_pos, d_neg


KGE_ANY_RELATION = 1 << 62                                                     # gn_kge_candidates_sample without a filter reads no relation table


def candidate_table(candidates, num_relations, device):
    """The per-relation candidate ranges of a ranged call, checked (ValueError) and contiguous: an int64 [num_relations, 2]
    tensor on `device` (num_relations None: whatever the table has); None stays None.  The values are read on the device."""
    if candidates is None:
        return None
    if not isinstance(candidates, torch.Tensor) or candidates.dtype != torch.int64 or candidates.dim() != 2 or \
            candidates.shape[1] != 2 or (num_relations is not None and candidates.shape[0] != num_relations) or \
            candidates.device != device:
        raise ValueError("`candidates` must be an int64 [{}, 2] tensor on {}, got {}".format(
            "R" if num_relations is None else num_relations, device,
            "{} {} on {}".format(candidates.dtype, tuple(candidates.shape), candidates.device)
            if isinstance(candidates, torch.Tensor) else type(candidates).__name__))
    return candidates if candidates.is_contiguous() else candidates.contiguous()


def kge_candidates_sample(fixed, et, k, nentity, known, seed, step, out, candidates=None):
    """gn_kge_candidates_sample_ranged: `out` (int64 [B, k], unit inner stride) = k candidates per (fixed[b], et[b]) that are
    not partners of `known`'s row (None: no filter), from the range `candidates` gives the relation (int64 [R, 2]; None: every
    entity).  Bad ids: a row of -1 and the device's error flag."""
    fixed, types = i64_vec(fixed), i64_vec(et)
    b = int(fixed.numel())
    candidates = candidate_table(candidates, None if known is None else known.num_et, fixed.device)
    nrel = known.num_et if known is not None else KGE_ANY_RELATION if candidates is None else int(candidates.shape[0])
    _call("gn_kge_candidates_sample_ranged", ptr(fixed), ptr(types), b, int(k), int(nentity), nrel, None if known is None else known._h,
          int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step), ptr(out), ld(out), ptr(error_flag(fixed.device)), stream_ptr(fixed.device),
          ptr(candidates))
    return out


GAT_MAX_ROW = 128                                                              # GN_GAT_MAX_ROW: floats of a row (heads x channels)


def gat_forward(plan, h, att, heads, negative_slope, bias, concat, relu, out, o_save=None):
    """gn_gat_logits_f32 + gn_gat_forward_f32: the attention layer's output into `out` from h = x W [N, heads * C] (contiguous)
    over `plan` (GraphPlan.gcn of the edge list: its working list is the layer's).  Returns (a_dst, a_src, m, rinv), [N, heads]
    each, what the backward recomputes alpha from; `o_save` [N, heads * C] receives the output before mean, bias and ReLU."""
    n, f = h.shape
    c = f // heads
    dev = h.device
    a_dst, a_src, m, rinv = (torch.empty((n, heads), dtype=torch.float32, device=dev) for _ in range(4))
    _call("gn_gat_logits_f32", ptr(h), ld(h), n, heads, c, ptr(att), ptr(a_dst), ptr(a_src), stream_ptr(dev))
    _call("gn_gat_forward_f32", plan._h, ptr(h), ld(h), heads, c, ptr(a_dst), ptr(a_src), float(negative_slope), ptr(bias),
          int(bool(concat)), int(bool(relu)), ptr(out), ld(out), ptr(o_save), ptr(m), ptr(rinv), stream_ptr(dev))
    return a_dst, a_src, m, rinv


def gat_backward(plan, h, att, heads, negative_slope, concat, g, o, a_dst, a_src, m, rinv):
    """(dh [N, heads * C], d_att like `att`) from g = dL/d(output before bias and ReLU): [N, heads * C], or [N, C] for the head
    mean.  gn_gat_backward_dst_f32, gn_gat_backward_src_f32 (the plan's source-major CSR must exist: `build_transpose`) and
    gn_gat_att_grad_f32; every sum in a fixed order."""
    n, f = h.shape
    c = f // heads
    dev = h.device
    pack = torch.empty((n, heads, 4), dtype=torch.float32, device=dev)
    da_dst, da_src = torch.empty((n, heads), dtype=torch.float32, device=dev), torch.empty((n, heads), dtype=torch.float32, device=dev)
    dh, d_att = torch.empty_like(h), torch.empty_like(att)
    slope, cc = float(negative_slope), int(bool(concat))
    _call("gn_gat_backward_dst_f32", plan._h, ptr(h), ld(h), heads, c, ptr(a_dst), ptr(a_src), ptr(m), ptr(rinv), slope, ptr(g), ld(g),
          cc, ptr(o), ptr(pack), ptr(da_dst), stream_ptr(dev))
    _call("gn_gat_backward_src_f32", plan._h, ptr(h), ld(h), heads, c, ptr(a_src), ptr(pack), slope, ptr(g), ld(g), cc, ptr(da_dst),
          ptr(att), ptr(dh), ld(dh), ptr(da_src), stream_ptr(dev))
    need = int(load().gn_gat_att_grad_workspace_bytes(n, heads, c))
    ws = torch.empty((max(need, 4),), dtype=torch.uint8, device=dev)
    _call("gn_gat_att_grad_f32", ptr(h), ld(h), n, heads, c, ptr(da_dst), ptr(da_src), ptr(d_att), ptr(ws), need, stream_ptr(dev))
    return dh, d_att


def link_loss_forward(pos, neg, eps):
    """``-mean(log(pos + eps)) - mean(log(1 - neg + eps))`` of two contiguous fp32 score vectors, a 0-d tensor
    (gn_link_loss_forward_f32; its per-device scratch is zeroed once: the kernel leaves it ready for the next launch)."""
    loss = torch.empty((), dtype=torch.float32, device=pos.device)
    ws = zeroed_once(pos.device, "link loss", load().gn_link_loss_workspace_bytes)
    _call("gn_link_loss_forward_f32", ptr(pos), pos.numel(), ptr(neg), neg.numel(), float(eps), ptr(loss), ptr(ws), ws.numel(),
          stream_ptr(pos.device))
    return loss


def link_loss_backward(pos, neg, eps, g):
    """(d loss / d pos, d loss / d neg) of `link_loss_forward` times the upstream gradient `g` (a contiguous fp32 scalar on
    the device): gn_link_loss_backward_f32."""
    dp, dn = torch.empty_like(pos), torch.empty_like(neg)
    _call("gn_link_loss_backward_f32", ptr(pos), pos.numel(), ptr(neg), neg.numel(), float(eps), ptr(g), ptr(dp), ptr(dn),
          stream_ptr(pos.device))
    return dp, dn


class NegativeSampler(Handle):
    """Device-side typed negative sampling for one static positive edge list (reference:
    gripnet/utils.py:98-119, called once per epoch at GripNet-pose.py:131).

        sampler = NegativeSampler(data.train_idx, n_d_node, data.train_range)
        neg_index = sampler.sample(seed=epoch)          # [2, E] int64 on the GPU, no host round trip
    """
    _destroy = "gn_negative_sampler_destroy"

    def __init__(self, pos_edge_index, num_nodes, range_list=None):
        load()
        require_gpu(pos_edge_index)
        ei, u, v, e = edge_rows(pos_edge_index)
        if range_list is None:
            range_list = [[0, e]]
        rl = torch.as_tensor(range_list).to("cpu", torch.int64).contiguous().view(-1, 2)
        self._create("gn_negative_sampler_create", ei.device, u, v, rl.data_ptr(), rl.shape[0], e, int(num_nodes))
        self.device, self.num_edges, self.num_nodes = ei.device, e, int(num_nodes)

    def sample(self, seed: int = 0, out=None, step=None) -> torch.Tensor:
        """[2, E] int64 negative pairs.  For graphs of up to 65,535 nodes the same launch also leaves every pair as one
        32-bit word; it travels with the returned tensor (`_gn_packed`) and the decoder scores the list from it - 6
        instead of 24 bytes per edge - as long as the tensor is not modified.

        `step`: a one-element int64 tensor on the device.  The draw then is the one of ``seed + step`` and the counter is
        advanced by one behind it, on the device: a CAPTURED training step that contains this call draws new negatives at
        every replay (gn_negative_sampler_sample_stepped)."""
        if step is not None and (step.dtype != torch.int64 or step.numel() != 1 or step.device != self.device):
            raise ValueError("`step` must be a one-element int64 tensor on {}".format(self.device))
        if out is None:
            out = torch.empty((2, self.num_edges), dtype=torch.int64, device=self.device)
        elif tuple(out.shape) != (2, self.num_edges) or out.dtype != torch.int64 or not out.is_contiguous() or out.device != self.device:
            raise ValueError("`out` must be a contiguous [2, {}] int64 tensor on {}".format(self.num_edges, self.device))
        else:
            out._gn_volatile = True          # refilled behind torch's back (`_version` does not move): never a static list
        base, packed = out.data_ptr(), None
        if self.num_nodes <= 65535 and self.num_edges > 0:
            # (a refilled `out` keeps its packed words' buffer: a captured step that scores `out` replays on the new draw)
            held = getattr(out, "_gn_packed", None)
            packed = held[0] if held is not None else torch.empty((self.num_edges,), dtype=torch.int32, device=self.device)
        head = (self._h, int(seed) & 0xFFFFFFFFFFFFFFFF)
        pairs = (base, base + 8 * self.num_edges)
        tail = (ptr(error_flag(self.device)), stream_ptr(self.device))
        if step is not None:
            _call("gn_negative_sampler_sample_stepped", *head, ptr(step), *pairs, ptr(packed), *tail)
        elif packed is not None:
            _call("gn_negative_sampler_sample_packed", *head, *pairs, ptr(packed), *tail)
        else:
            _call("gn_negative_sampler_sample", *head, *pairs, *tail)
        if packed is not None:
            out._gn_packed = (packed, out._version)
        return out


class KnownPairs(Handle):
    """Owner of a gn_known_pairs handle: the union of one or more (edge_index [2,E], edge_type [E]) int64 lists on the GPU
    (train + test, typically) as the filter of filtered ranking (multiRelaInnerProductDecoder.rank / top_k).  Duplicates
    are allowed (set semantics); ids are validated here (IndexError).  One sorted partner row per (relation, u): O(E + R n)
    memory, whatever n.  Built once; the ranking calls that use it neither synchronise nor allocate.

        known = KnownPairs([(data.train_idx, data.train_et), (data.test_idx, data.test_et)], n_d, num_et)
    """
    _destroy = "gn_known_pairs_destroy"

    def __init__(self, lists, num_nodes, num_et):
        load()
        if isinstance(lists, tuple) and len(lists) == 2 and torch.is_tensor(lists[0]):
            lists = [lists]
        lists = list(lists)
        if not lists:
            raise ValueError("KnownPairs needs at least one (edge_index, edge_type) list")
        rows, types = [], []
        for edge_index, edge_type in lists:
            require_gpu(edge_index, edge_type)
            if edge_index.dim() != 2 or edge_index.shape[0] != 2:
                raise ValueError("edge_index must have shape [2, E], got {}".format(tuple(edge_index.shape)))
            if edge_type.dim() != 1 or edge_type.shape[0] != edge_index.shape[1]:
                raise ValueError("edge_type has {} entries for {} edges".format(edge_type.numel(), edge_index.shape[1]))
            rows.append(i64_vec(edge_index))
            types.append(i64_vec(edge_type))
        device = rows[0].device
        if any(t.device != device for t in rows + types):
            raise ValueError("KnownPairs: every list must be on one device")
        ei = torch.cat(rows, dim=1).contiguous() if len(rows) > 1 else rows[0].contiguous()
        et = torch.cat(types).contiguous() if len(types) > 1 else types[0]
        e = int(ei.shape[1])
        self._create("gn_known_pairs_create", device, ei.data_ptr(), ei.data_ptr() + 8 * e, et.data_ptr(), e, int(num_nodes), int(num_et))
        self.device, self.num_edges, self.num_nodes, self.num_et = device, e, int(num_nodes), int(num_et)


def _known_handle(known, z, weight):
    if known is None:
        return None
    if not isinstance(known, KnownPairs):
        raise TypeError("`known` must be a KnownPairs, got {}".format(type(known).__name__))
    if known.num_nodes != z.shape[0] or known.num_et != weight.shape[0] or known.device != z.device:
        raise ValueError("KnownPairs was built for {} nodes / {} relations on {}; the call has {} / {} on {}".format(
            known.num_nodes, known.num_et, known.device, z.shape[0], weight.shape[0], z.device))
    return known._h


def distmult_rank(z, edge_index, edge_type, weight, known=None, candidates=None):
    """(greater, ties) int32 [E]: per pair (u, v, r) the non-known candidates v' != v scored not below-or-equal / equal to (u, v, r)
    (gn_distmult_rank_ranged_f32; a NaN on either side counts as greater).  `z` rows contiguous fp32.  `candidates`: int64 [R, 2] ranges per relation, or None."""
    candidates = candidate_table(candidates, weight.shape[0], z.device)
    ei, u, v, e = edge_rows(edge_index)
    et = i64_vec(edge_type)
    if et.numel() != e:
        raise ValueError("edge_type has {} entries for {} edges".format(et.numel(), e))
    greater = torch.empty((e,), dtype=torch.int32, device=z.device)
    ties = torch.empty((e,), dtype=torch.int32, device=z.device)
    _call("gn_distmult_rank_ranged_f32", ptr(z), ld(z), z.shape[0], z.shape[1], ptr(weight), ld(weight), weight.shape[0], u, v,
          ptr(et), e, _known_handle(known, z, weight), ptr(greater), ptr(ties), ptr(error_flag(z.device)), stream_ptr(z.device),
          ptr(candidates))
    return greater, ties


def distmult_topk(z, nodes, edge_type, weight, k, known=None, candidates=None):
    """(scores fp32 [Q, k], partners int64 [Q, k]) of the queries (nodes[q], edge_type[q]) (gn_distmult_topk_ranged_f32)."""
    candidates = candidate_table(candidates, weight.shape[0], z.device)
    nodes, et = i64_vec(nodes), i64_vec(edge_type)
    if nodes.dim() != 1 or et.dim() != 1 or nodes.numel() != et.numel():
        raise ValueError("nodes and edge_type must be 1-D of one length, got {} and {}".format(tuple(nodes.shape), tuple(et.shape)))
    q = int(nodes.numel())
    scores = torch.empty((q, k), dtype=torch.float32, device=z.device)
    ids = torch.empty((q, k), dtype=torch.int64, device=z.device)
    _call("gn_distmult_topk_ranged_f32", ptr(z), ld(z), z.shape[0], z.shape[1], ptr(weight), ld(weight), weight.shape[0], ptr(nodes),
          ptr(et), q, int(k), _known_handle(known, z, weight), ptr(scores), ptr(ids), ptr(error_flag(z.device)),
          stream_ptr(z.device), ptr(candidates))
    return scores, ids


KGE_SHARED_MAX_ROW = 128                                                       # floats of an entity row the shared-list kernels take (the ranking limit)
KGE_SIDES = {"tail": 0, "head": 1}                                             # GN_KGE_SIDE_* of include/gripnet_hip.h
KGE_RANK_MAX_ROW = 128                                                         # floats of an entity row the ranking kernels take


def _kge_rank_operands(model, ent, rel, side, known, queries):
    """(model id, side id, hidden size, known handle, workspace, its size) of a KGE ranking call, shapes checked."""
    if side not in KGE_SIDES:
        raise ValueError("side must be 'tail' or 'head', got {!r}".format(side))
    m = KGE_MODELS[model]
    h = rel.shape[1] // 2 if model == "ComplEx" else rel.shape[1]
    de = 2 * h if model in ("ComplEx", "RotatE") else h
    if ent.shape[1] != de or (model == "ComplEx" and rel.shape[1] != 2 * h):
        raise ValueError("{}: entity rows of {} and relation rows of {} columns do not belong together".format(
            model, ent.shape[1], rel.shape[1]))
    if de > KGE_RANK_MAX_ROW:
        raise ValueError("{}: the ranking kernels take entity rows of at most {} floats (hidden_dim <= {}), got {}".format(
            model, KGE_RANK_MAX_ROW, KGE_RANK_MAX_ROW * h // de, de))
    need = int(load().gn_kge_rank_workspace_bytes(m, rel.shape[0], h, queries))
    ws = torch.empty((need,), dtype=torch.uint8, device=ent.device) if need else None
    return m, KGE_SIDES[side], h, _known_handle(known, ent, rel), ws, need


def kge_rank(model, ent, rel, sample, et, gamma, divisor, side="tail", known=None, candidates=None):
    """(greater, ties) int32 [E] of the triples (sample[0, e], et[e], sample[1, e]) against every candidate tail (`side`
    "tail") or head ("head") that is not in `known` (gn_kge_rank_ranged_f32).  `ent`, `rel`: rows contiguous fp32.
    `candidates`: int64 [R, 2] ranges per relation for that side, or None."""
    candidates = candidate_table(candidates, rel.shape[0], ent.device)
    idx, head, tail, e = edge_rows(sample)
    types = i64_vec(et)
    if types.numel() != e:
        raise ValueError("edge_type has {} entries for {} triples".format(types.numel(), e))
    m, sd, h, kh, ws, need = _kge_rank_operands(model, ent, rel, side, known, e)
    fixed, truth = (head, tail) if sd == 0 else (tail, head)
    greater = torch.empty((e,), dtype=torch.int32, device=ent.device)
    ties = torch.empty((e,), dtype=torch.int32, device=ent.device)
    _call("gn_kge_rank_ranged_f32", m, sd, ptr(ent), ld(ent), ent.shape[0], ptr(rel), ld(rel), rel.shape[0], h, fixed, truth, ptr(types), e,
          float(gamma), float(divisor), kh, ptr(greater), ptr(ties), ptr(error_flag(ent.device)), ptr(ws), need,
          stream_ptr(ent.device), ptr(candidates))
    return greater, ties


def kge_topk(model, ent, rel, entities, et, k, gamma, divisor, side="tail", known=None, candidates=None):
    """(scores fp32 [Q, k], ids int64 [Q, k]) of the queries (entities[q], et[q]) (gn_kge_topk_ranged_f32)."""
    candidates = candidate_table(candidates, rel.shape[0], ent.device)
    entities, types = i64_vec(entities), i64_vec(et)
    if entities.dim() != 1 or types.dim() != 1 or entities.numel() != types.numel():
        raise ValueError("entities and edge_type must be 1-D of one length, got {} and {}".format(
            tuple(entities.shape), tuple(types.shape)))
    q = int(entities.numel())
    m, sd, h, kh, ws, need = _kge_rank_operands(model, ent, rel, side, known, q)
    scores = torch.empty((q, k), dtype=torch.float32, device=ent.device)
    ids = torch.empty((q, k), dtype=torch.int64, device=ent.device)
    _call("gn_kge_topk_ranged_f32", m, sd, ptr(ent), ld(ent), ent.shape[0], ptr(rel), ld(rel), rel.shape[0], h, ptr(entities), ptr(types), q,
          int(k), float(gamma), float(divisor), kh, ptr(scores), ptr(ids), ptr(error_flag(ent.device)), ptr(ws), need,
          stream_ptr(ent.device), ptr(candidates))
    return scores, ids


class MetricsPlan(Handle):
    """Owner of a gn_link_metrics_plan handle: the segments of one range list (what relation_metrics needs besides the scores)."""
    _destroy = "gn_link_metrics_plan_destroy"

    def __init__(self, range_list, device):
        rl = torch.as_tensor(range_list).to("cpu", torch.int64).contiguous().view(-1, 2)
        self.R = int(rl.shape[0])
        self.E = int(rl[-1, 1]) if self.R else 0
        self.device = torch.device(device)
        self._create("gn_link_metrics_plan_create", self.device, rl.data_ptr(), self.R, self.E)
        self.workspace_bytes = int(load().gn_link_metrics_plan_workspace_bytes(self._h))
        self._ws = None

    def workspace(self):
        if self._ws is None:
            self._ws = torch.empty((max(self.workspace_bytes, 1),), dtype=torch.uint8, device=self.device)
        return self._ws


_range_plans = VersionedCache(4)      # (range_list tensor, device) -> MetricsPlan


def metrics_plan(range_list, device):
    """The MetricsPlan of a range list, kept while the same tensor (unmodified) keeps coming: an epoch loop's train / test
    ranges (a list / array has no version to watch: not kept)."""
    dev = torch.device(device)
    plan = _range_plans.get(range_list, dev)
    return _range_plans.put(range_list, MetricsPlan(range_list, dev), dev) if plan is MISS else plan


def link_metrics(pos_score, neg_score, range_list):
    """(auprc, auroc, ap), each a float64 [R] tensor on the GPU: scikit-learn's three link-prediction
    metrics for every relation block at once (reference: one sklearn call per relation and epoch).  Asynchronous.
    Scores are compared as fp32 values, so -0.0 and +0.0 tie; NaN and +-inf are the caller's to exclude (scikit-learn raises on them)."""
    require_gpu(pos_score, neg_score)
    pos = pos_score.detach().to(torch.float32).contiguous()
    neg = neg_score.detach().to(torch.float32).contiguous()
    if pos.numel() != neg.numel():
        raise ValueError("positive and negative score lists differ in length")
    plan = metrics_plan(range_list, pos.device)
    if plan.E != int(pos.numel()):
        raise ValueError("range_list covers {} edges, {} scores given".format(plan.E, int(pos.numel())))
    out = torch.empty((3, plan.R), dtype=torch.float64, device=pos.device)
    ws = plan.workspace()
    _call("gn_link_metrics_planned_f32", plan._h, ptr(pos), ptr(neg), ptr(out), ptr(ws), ws.numel(), stream_ptr(pos.device))
    return out[0], out[1], out[2]


MAX_CLASSES = 1024                                      # num_class limit of gn_class_metrics_f32


def _class_metrics_args(score_or_pred, classes, num_class=None):
    """(score mode?, num_class) of a class_metrics call, checked without touching a device: a 2-D fp32 score matrix
    (num_class defaults to its width and must equal it) or a 1-D int64 vector of predicted ids (num_class required),
    and int64 class ids of the same length."""
    x = score_or_pred
    if num_class is not None and not isinstance(num_class, bool):
        try:
            num_class = operator.index(num_class)                  # (numpy and torch integers too; a float is refused below)
        except TypeError:
            pass
    if not isinstance(x, torch.Tensor) or not isinstance(classes, torch.Tensor):
        raise TypeError("class_metrics takes tensors, got {} and {}".format(type(x).__name__, type(classes).__name__))
    if x.dim() == 2:
        if x.dtype != torch.float32:
            raise TypeError("class scores must be fp32, got {}".format(x.dtype))
        width = int(x.shape[1])
        if num_class is None:
            num_class = width
        elif num_class != width:
            raise ValueError("num_class {!r} differs from the score matrix's width {}".format(num_class, width))
        score_mode = True
    elif x.dim() == 1:
        if x.dtype != torch.int64:
            raise TypeError("predicted class ids must be int64 (torch.long), got {}".format(x.dtype))
        if num_class is None:
            raise ValueError("num_class is required with predicted class ids")
        score_mode = False
    else:
        raise ValueError("expected a [n, C] score matrix or [n] predicted ids, got shape {}".format(tuple(x.shape)))
    if not isinstance(num_class, int) or isinstance(num_class, bool) or not 1 <= num_class <= MAX_CLASSES:
        raise ValueError("num_class must be an int in [1, {}], got {!r}".format(MAX_CLASSES, num_class))
    if classes.dtype != torch.int64:
        raise TypeError("class ids must be int64 (torch.long), got {}".format(classes.dtype))
    if classes.dim() != 1 or classes.shape[0] != x.shape[0]:
        raise ValueError("classes must be a [{}] vector, got shape {}".format(int(x.shape[0]), tuple(classes.shape)))
    return score_mode, num_class


def class_metrics(score_or_pred, classes, num_class=None):
    """(pred int64 [n] or None, counts int64 [3, C], per_class float64 [3, C], summary float64 [3]) on the GPU
    (gn_class_metrics_f32): argmax of a score matrix (or given predicted ids), per-class support / predicted / correct,
    precision / recall / F1, and micro-F1 / macro-F1 / accuracy.  Asynchronous and capturable: an out-of-range class id
    sets bit 3 (value 8) of the error word (raise_if_index_errors) and makes every float64 output NaN."""
    score_mode, C = _class_metrics_args(score_or_pred, classes, num_class)
    require_gpu(score_or_pred, classes)
    dev = score_or_pred.device
    if classes.device != dev:
        raise ValueError("scores and classes are on different devices: {} and {}".format(dev, classes.device))
    y = i64_vec(classes)
    n = int(y.shape[0])
    if score_mode:
        x = f32_rows(score_or_pred.detach())
        pred = torch.empty((n,), dtype=torch.int64, device=dev)
        args = (ptr(x), ld(x), None)
    else:
        x = i64_vec(score_or_pred)
        pred = None
        args = (None, 0, ptr(x))
    counts = torch.empty((3, C), dtype=torch.int64, device=dev)
    per_class = torch.empty((3, C), dtype=torch.float64, device=dev)
    summary = torch.empty((3,), dtype=torch.float64, device=dev)
    ws = torch.empty((int(load().gn_class_metrics_workspace_bytes(n, C)),), dtype=torch.uint8, device=dev)
    _call("gn_class_metrics_f32", *args, ptr(y), n, C, ptr(pred), ptr(counts), ptr(per_class), ptr(summary),
          ptr(error_flag(dev)), ptr(ws), ws.numel(), stream_ptr(dev))
    return pred, counts, per_class, summary


def class_scores(z, weight, nodes, out, softmax=True):
    """out = softmax?(z[nodes] @ weight) in one launch (gn_class_scores_f32)."""
    _call("gn_class_scores_f32", ptr(z), ld(z), z.shape[0], ptr(nodes), out.shape[0], ptr(weight), ld(weight),
          weight.shape[0], weight.shape[1], int(bool(softmax)), ptr(out), ld(out), stream_ptr(z.device))
    return out


def softmax_rows(x):
    _call("gn_softmax_rows_f32", ptr(x), ld(x), x.shape[0], x.shape[1], stream_ptr(x.device))
    return x
