"""ctypes binding of libparq_hip.so (include/parq_hip.h).

The product path has NO fallback: if the HIP library is missing or a symbol
cannot be resolved, importing callers get a RuntimeError that says how to build
it.  ``import torch`` must come first so that the process-wide HIP runtime
(torch's bundled libamdhip64.so.7) is the one our kernels register with.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (loads the HIP runtime before our library)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_C", "libparq_hip.so")
# development build (-DPARQ_DEV_PROBES: environment A/B switches, probe kernels, in-kernel time stamps).  Never loaded by the
# package itself: tools/ and `bench.py --dev-lib` opt in with use_dev_library() before the first load().
DEV_LIB_PATH = os.path.join(_HERE, "_C", "libparq_hip_dev.so")

PROF_KV_PROJ, PROF_PROJECT_SAMPLE, PROF_CROSS_ATTN, PROF_SELF_ATTN, PROF_LINEAR, PROF_OTHER, PROF_MERGE = range(7)
PROF_NAMES = ["kv_proj", "project_sample", "cross_attn", "self_attn", "linear", "other", "cross_attn_merge"]


class ParqConfig(C.Structure):
    _fields_ = [("dim", C.c_int32), ("num_queries", C.c_int32), ("num_classes", C.c_int32),
                ("num_heads", C.c_int32), ("ffn_dim", C.c_int32), ("num_layers", C.c_int32),
                ("share_weights", C.c_int32), ("num_mean_sizes", C.c_int32), ("scale", C.c_float * 6)]


class ParqScene(C.Structure):
    _fields_ = [("B", C.c_int32), ("V", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("tokens", C.c_void_p), ("camera", C.c_void_p), ("T_camera_pseudoCam", C.c_void_p),
                ("T_world_pseudoCam", C.c_void_p), ("T_world_local", C.c_void_p)]


class ParqOutputs(C.Structure):
    _fields_ = [("pred_logits", C.c_void_p), ("center_unnormalized", C.c_void_p),
                ("size_unnormalized", C.c_void_p), ("ortho6d", C.c_void_p),
                ("sem_cls_prob", C.c_void_p), ("coord_pos", C.c_void_p)]


class ParqOutputGrads(C.Structure):
    _fields_ = [("pred_logits", C.c_void_p), ("center_unnormalized", C.c_void_p),
                ("size_unnormalized", C.c_void_p), ("ortho6d", C.c_void_p)]


class ParqFpnLevels(C.Structure):
    _fields_ = [("level", C.c_void_p * 4), ("h", C.c_int32 * 4), ("w", C.c_int32 * 4), ("layer", C.c_int32)]


# every symbol include/parq_hip.h declares: (restype, argtypes)
_vp, _i32, _i64, _sz, _f = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_float
SYMBOLS = {
    "parq_last_error": (C.c_char_p, []),
    "parq_version": (C.c_char_p, []),
    "parq_create": (C.c_int, [C.POINTER(ParqConfig), C.POINTER(_vp)]),
    "parq_destroy": (C.c_int, [_vp]),
    "parq_set_weight": (C.c_int, [_vp, C.c_char_p, _vp, _i64]),
    "parq_packed_weights_bytes": (_sz, [_vp]),
    "parq_pack_weights": (C.c_int, [_vp, _vp, _sz, _vp]),
    "parq_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32]),
    "parq_forward": (C.c_int, [_vp, C.POINTER(ParqScene), _vp, _sz, C.POINTER(ParqOutputs), _vp]),
    "parq_forward_capture": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp, C.POINTER(_vp)]),
    "parq_forward_replay": (C.c_int, [_vp, _vp, C.POINTER(ParqScene), _vp, _sz, C.POINTER(ParqOutputs), _vp]),
    "parq_graph_nodes": (_i64, [_vp]),
    "parq_graph_destroy": (C.c_int, [_vp]),
    "parq_prepare": (C.c_int, [_vp, C.POINTER(ParqScene), _vp, _sz, _vp]),
    "parq_iterate": (C.c_int, [_vp, C.POINTER(ParqScene), _vp, _sz, _i32, _vp, C.POINTER(ParqOutputs), _vp, _vp]),
    "parq_attention_map_scratch_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32, _i32]),
    "parq_attention_map": (C.c_int, [_vp, C.POINTER(ParqScene), _vp, _sz, _vp, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "parq_workspace_lookup": (C.c_int, [_vp, _i32, _i32, _i32, _i32, C.c_char_p, C.POINTER(_sz), C.POINTER(_sz)]),
    "parq_set_attention_mode": (C.c_int, [_vp, _i32]),
    "parq_set_token_type": (C.c_int, [_vp, _i32]),
    "parq_set_train_token_type": (C.c_int, [_vp, _i32]),
    "parq_set_head_tiers": (C.c_int, [_vp, C.c_uint32, _i32]),
    "parq_set_seam_fusion": (C.c_int, [_vp, _i32]),
    "parq_set_range_mirror": (C.c_int, [_vp, _vp]),
    "parq_mirror_take": (_i32, [_vp]),
    "parq_set_progress": (C.c_int, [_vp, _vp, _i32]),
    "parq_shard_exchange_floats": (_sz, [_vp, _i32, _i32]),
    "parq_iterate_sharded": (C.c_int, [_vp, C.POINTER(ParqScene), _vp, _sz, _i32, _i32, _vp, C.POINTER(ParqOutputs), _vp, _vp, _vp, _i32, _vp]),
    "parq_profile_enable": (C.c_int, [_vp, _i32]),
    "parq_profile_read": (C.c_int, [_vp, _i32, C.POINTER(C.c_double), C.POINTER(_i64)]),
    "parq_set_dropout": (C.c_int, [_vp, _f, C.c_uint32]),
    "parq_set_backward_batched": (C.c_int, [_vp, _i32]),
    "parq_k_dropout_mask": (C.c_int, [_vp, _i32, _i32, _i64, _i64, _vp, _vp]),
    "parq_train_workspace_bytes": (_sz, [_vp, _i32, _i32, _i32, _i32]),
    "parq_grad_arena_bytes": (_sz, [_vp]),
    "parq_forward_train": (C.c_int, [_vp, C.POINTER(ParqScene), _vp, _sz, C.POINTER(ParqOutputs), _vp]),
    "parq_wait_iteration": (C.c_int, [_vp, C.c_int32]),
    "parq_backward": (C.c_int, [_vp, C.POINTER(ParqScene), _vp, _sz, C.POINTER(ParqOutputs), C.POINTER(ParqOutputGrads), _vp, _vp, _vp]),
    "parq_arena_lookup": (C.c_int, [_vp, C.c_char_p, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "parq_grad_bucket": (C.c_int, [_vp, _i32, C.POINTER(_i64), C.POINTER(_i64)]),
    "parq_backward_wait_bucket": (C.c_int, [_vp, _i32, _vp]),
    "parq_set_backward_streams": (C.c_int, [_vp, _i32]),
    "parq_set_deterministic": (C.c_int, [_vp, _i32]),
    "parq_ray_pe_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "parq_ray_pe_workspace_bytes_flags": (_sz, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "parq_ray_pe": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f), _f, _f, _i32, _i32, _i32, _i32, _i32, _i32,
                              _vp, _vp, _i32, _vp, _sz, _vp]),
    "parq_ray_pe_fpn": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f), _f, _f, _i32, _i32, _i32, _i32, _i32, _i32,
                                  C.POINTER(ParqFpnLevels), _vp, _i32, _vp, _sz, _vp]),
    "parq_fpn_backward": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(ParqFpnLevels), C.POINTER(_vp), _vp]),
    "parq_ray_pe_backward_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "parq_ray_pe_backward": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_f), _f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                       _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "parq_ray_pe_backward_workspace_bytes_flags": (_sz, [_i32, _i32, _i32, _i32, _i32, _i32, _i32]),
    "parq_ray_pe_backward_flags": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_f), _f, _f, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp,
                                             _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "parq_parse_pred": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, C.POINTER(_f), _i32, _i32, _vp, _vp, _vp]),
    "parq_obb_iou": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i32, _i64, _vp, _vp, _vp]),
    "parq_set_loss": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp,
                                C.POINTER(_f), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "parq_set_loss_scratch_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "parq_set_loss_flags": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp,
                                      C.POINTER(_f), _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "parq_k_project_sample": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(_f), _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "parq_k_camera_local": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "parq_k_linear": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "parq_k_linear_half": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "parq_k_attention_scratch_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "parq_k_attention": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "parq_k_attention_split_scratch_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "parq_k_attention_split": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "parq_k_attention_split8": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "parq_k_attention_split256_scratch_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "parq_k_attention_split256": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "parq_k_attention_half_scratch_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "parq_k_attention_half": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "parq_k_layernorm": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _f, _vp]),
}

# entry points added since: typed by load() like the table above (whose size tests/test_train_token16_cpu.py pins)
EXTRA_SYMBOLS = {
    "parq_set_batch_invariant": (C.c_int, [_vp, _i32]),
    "parq_forward_views": (C.c_int, [_vp, _vp, C.POINTER(ParqScene), _vp, _sz, C.POINTER(ParqOutputs), C.POINTER(_i32), _i32,
                                     C.POINTER(_i64), _vp]),
    "parq_draw_boxes_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "parq_draw_boxes": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp, _i32, _vp]),
    "parq_frame_plan_ints": (_sz, [_i32, _i32]),
    "parq_frame_plan": (C.c_int, [_i32, _i32, C.POINTER(_i32)]),
    "parq_frames_resize": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "parq_assign_max_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "parq_assign_max": (C.c_int, [_vp, _i64, _vp, _i32, _i32, _i32, _vp, _sz, _vp, _i64, _vp]),
    "parq_tracks_store_bytes": (_sz, [_i32, _i32]),
    "parq_tracks_update_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "parq_tracks_update": (C.c_int, [_vp, _i32, _i32, C.POINTER(_i32), _i32, _vp, _vp, _vp, _i32, _i32, _f, _f, _vp, _sz, _vp, _vp, _vp]),
    "parq_k_project_sample_backward_scratch_bytes": (_sz, [_i32, _i32, _i32]),
    "parq_k_project_sample_backward": (C.c_int, [_vp, _i32, _vp, _vp, _vp, C.POINTER(_f), _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                                 _vp, _sz, _vp]),
    "parq_k_attention_backward_scratch_bytes": (_sz, [_i32] * 7),
    "parq_k_attention_backward": (C.c_int, [_vp] * 6 + [_i32] * 8 + [_f, C.c_uint32, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp,
                                                                    C.POINTER(_i32), _vp]),
    "parq_k_attention_backward_batched": (C.c_int, [_vp] * 6 + [_i32] * 8 + [_f, C.POINTER(C.c_uint32), _vp, _vp, _vp, _sz, _vp, _vp,
                                                                            C.POINTER(_i32), _vp]),
}

# the matcher of the set loss (include/parq_hip.h parq_set_match): a third table, the sizes of the two above being pinned by tests
_u32 = C.c_uint32
MATCH_SYMBOLS = {
    "parq_set_match_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "parq_set_match": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _f, _f, _f, _i32, _u32, _u32, _u32, _vp, _sz,
                                 _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

# a snippet's training targets (include/parq_hip.h parq_snippet_targets): a fourth table, for the same reason
SNIPPET_SYMBOLS = {
    "parq_snippet_targets_workspace": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "parq_snippet_targets": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32,
                                       C.POINTER(_i32), C.POINTER(_f), _i32, _i32, _f, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp]),
}

ALL_TABLES = (SYMBOLS, EXTRA_SYMBOLS, MATCH_SYMBOLS, SNIPPET_SYMBOLS)

# the evaluator's ground-truth store and end-of-epoch counts (include/parq_hip.h parq_gt_tracks_update, parq_f1_counts): typed by load()
# like the tables above, but not a member of ALL_TABLES, whose total tests/test_snippets_cpu.py pins
EVAL_SYMBOLS = {
    "parq_gt_tracks_update_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "parq_gt_tracks_update": (C.c_int, [_vp, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, _vp, _vp, _vp, _i32, _f, C.c_uint64, _vp, _sz,
                                        _vp, _vp]),
    "parq_f1_counts_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "parq_f1_counts": (C.c_int, [_vp, _i32, _vp, _i32, _i32, C.POINTER(C.c_double), _i32, _i32, _vp, _sz, _vp, _vp, _vp, _vp]),
}

# the life record beside a track store (include/parq_hip.h parq_tracks_note, parq_tracks_retire): a table of its own for the same reason
LIFE_SYMBOLS = {
    "parq_tracks_life_bytes": (_sz, [_i32, _i32]),
    "parq_tracks_note": (C.c_int, [_vp, _vp, _i32, _i32, C.POINTER(_i32), _i32, _vp, _i32, _vp, _vp, _vp]),
    "parq_tracks_retire": (C.c_int, [_vp, _vp, _i32, _i32, C.POINTER(_i32), _i32, _i32, _i32, _i32, _vp, _vp]),
}

# average precision from the two track stores (include/parq_hip.h parq_average_precision): a table of its own for the same reason
AP_SYMBOLS = {
    "parq_average_precision_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "parq_average_precision": (C.c_int, [_vp, _i32, _vp, _i32, _i32, C.POINTER(C.c_double), _i32, _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _vp, _vp, _vp]),
}

_lib = None


def use_dev_library():
    """Development only (tools/, `bench.py --dev-lib`): bind the -DPARQ_DEV_PROBES build instead of the product library."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("parq_amd: use_dev_library() must be called before the library is first loaded")
    LIB_PATH = DEV_LIB_PATH


def is_dev_library():
    return LIB_PATH == DEV_LIB_PATH


def load():
    """Load libparq_hip.so (once) and type every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "parq_amd: HIP extension %s is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc, --offload-arch=gfx950). "
            "There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in [kv for table in ALL_TABLES + (EVAL_SYMBOLS, LIFE_SYMBOLS, AP_SYMBOLS) for kv in table.items()]:
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError("parq_amd: %s does not export %s (stale build?)" % (LIB_PATH, name)) from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().parq_last_error().decode("utf-8", "replace")
        raise RuntimeError("parq_amd: %s failed (code %d): %s" % (what, rc, msg))


def ptr(t):
    """Device pointer of a CUDA float32 contiguous tensor (or None)."""
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), \
        "expected a contiguous float32 CUDA tensor, got %s %s contiguous=%s" % (t.device, t.dtype, t.is_contiguous())
    return C.c_void_p(t.data_ptr())


def token_ptr(t):
    """Device pointer of the tokens of a scene: a contiguous CUDA tensor of float32, float16 or bfloat16 (parq_set_token_type)."""
    assert t.is_cuda and t.dtype in (torch.float32, torch.float16, torch.bfloat16) and t.is_contiguous(), \
        "expected contiguous float32 / float16 / bfloat16 CUDA tokens, got %s %s contiguous=%s" % (t.device, t.dtype, t.is_contiguous())
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
