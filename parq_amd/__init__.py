"""parq_amd — MI355X-native implementation of PARQ's recurrent pixel-aligned decoder path.

Public surface mirrors the reference (ymingxie/PARQ):
    PARQDecoder  (model/parq_decoder.py:30)      forward on the HIP kernel chain
    AddRayPE     (model/ray_positional_encoding.py:29)  ray-point PE (+ fused tokenisation)
    Pose, Camera (utils/wrappers.py:194,441)     tensor wrappers drivers pass in
    InFlight     (no counterpart: the reference calls its model once per batch, eval.py:46)  several forwards of one module in flight
    ViewWindow   (no counterpart: the reference re-projects every view of every snippet)  a streaming window of view slots
    draw_boxes, box_colors (utils/parq_utils.py:134,141 get_colors / draw_detections)  boxes drawn into the views on the device
    SceneTracks  (utils/f1_eval.py:293 matching_pred, there on the host and inside the evaluator only)  detections followed across
                 snippets in a device-resident track store: one enqueue per snippet batch returns a track id per query;
                 lifecycle=True (no counterpart) adds hits, age, stable uids and retire() for streams that never end
    f1_counts    (utils/f1_eval.py:36 count_matches over all scenes)  the evaluator's per-class counts from a prediction and a
                 ground-truth SceneTracks, on the device
    average_precision (no counterpart: the reference's evaluator has no AP)  AP per IoU threshold and class, and the curve behind
                 it, from the same two stores, on the device
    FramePrep, resize_frames, resized_intrinsics, gravity_aligned, snippet_local (datasets/transforms.py:211 ScanNetBaseTransform)
                 raw uint8 frames, intrinsics and T_world_camera prepared on the device into the batch PARQ.forward reads
    SnippetTargets, select_views (scripts/scannet_preprocessing/generate_scannet_anno_snippet.py, the offline annotation pass)
                 a snippet's obbs_padded / sym / num_valid from depth frames, intrinsics, poses and the scene's boxes, on the device
    ResnetFPN    (model/resnet_fpn.py:16)       wrapper of a user-supplied ResNet-FPN; its neck is fused into the tokenisation
The compute lives in ``parq_amd/_C/libparq_hip.so`` (C ABI: include/parq_hip.h).
"""
from .wrappers import Camera, Obb3D, Pose, TensorWrapper  # noqa: F401


def __getattr__(name):
    # lazy: importing the package must not require the HIP library (CPU-only tooling, synth)
    if name == "PARQDecoder":
        from .decoder import PARQDecoder
        return PARQDecoder
    if name == "AddRayPE":
        from .ray_pe import AddRayPE
        return AddRayPE
    if name == "PARQ":
        from .module import PARQ
        return PARQ
    if name == "ResnetFPN":
        from .resnet_fpn import ResnetFPN
        return ResnetFPN
    if name == "InFlight":
        from .inflight import InFlight
        return InFlight
    if name == "ViewWindow":
        from .view_window import ViewWindow
        return ViewWindow
    if name in ("draw_boxes", "box_colors"):
        from . import draw
        return getattr(draw, name)
    if name in ("SceneTracks", "f1_counts", "average_precision"):
        from . import scene_tracks
        return getattr(scene_tracks, name)
    if name in ("FramePrep", "resize_frames", "resized_intrinsics", "gravity_aligned", "snippet_local"):
        from . import frames
        return getattr(frames, name)
    if name in ("SnippetTargets", "select_views"):
        from . import snippets
        return getattr(snippets, name)
    raise AttributeError(name)
