"""A snippet's training targets from depth and poses, on the device (include/parq_hip.h parq_snippet_targets, csrc/snippets.hip).

The reference makes ``obbs_padded`` / ``sym`` of a snippet in an offline pass (scripts/scannet_preprocessing/
generate_scannet_anno_snippet.py over processing_utils.py): pick the frames of every snippet from the camera trajectory, count per
box the depth points inside it, measure how much of its projected extent lies inside the colour image, grade every box and keep
those that are visible enough.  Here:

    select_views     the four frame-selection rules (processing_utils.py:352-505), on the host in NumPy: a few hundred poses
    SnippetTargets   the per-snippet targets, two launches on the current stream: counts, truncation ratios, levels, the valid
                     rows compacted into ``obbs_padded`` / ``sym`` / ``num_valid``: ``batch.update(targets(...))`` after ``FramePrep``

Depth decoding, the Scan2CAD parse that gives the scene's box list, and dropping snippets with ``num_valid == 0`` (a read-back
the caller chooses when to pay) stay the caller's.  The rule is stated in full in include/parq_hip.h and INTEGRATION.md "Targets
from depth".
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .wrappers import Obb3D, raw

MAX_BOXES = 128            # boxes of a scene
MAX_FRAMES = 64            # frames of a snippet
MAX_SCENES = 1023
MAX_SIDE = 8192            # every side of a depth frame and of the colour image
MAX_LEVELS = 8
DEFAULT_LEVELS = ((1000, 0.85), (500, 0.70), (100, 0.50))          # the reference's get_level: (points above, ratio above) per level
MODES = ("val", "w1", "train", "all")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _is_num(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


# ---- frame selection (host) -----------------------------------------------------------------------------------------------------
def select_views(T_world_camera, mode, window_size=3, min_angle=15.0, min_distance=0.1):
    """Lists of frame ids, one list per snippet: the reference's frame selection over a camera trajectory.

    ``T_world_camera``: ``(n, 4, 4)`` poses by frame id, or a dict ``{id: (4, 4)}`` in id order.  A frame whose pose is not finite is
    skipped.  A frame is a key frame when the camera's forward axis turned by more than ``min_angle`` degrees or the camera moved by
    more than ``min_distance`` since the last key frame (the first finite frame is one).  ``mode``:

        "val"    consecutive groups of ``window_size`` key frames (view_selection)
        "w1"     every key frame alone (view_selection_w1)
        "train"  every window of ``window_size`` consecutive key frames, shifted by 0..9 frames where all shifted frames exist and the
                 last does not pass the last frame; duplicates removed in first-seen order (view_selection_overlap)
        "all"    one list of all key frames (view_selection_allframes)

    The angle is ``arccos`` of the (2, 2) entry of ``inv(R) @ R_last``; an argument that rounds above 1 gives NaN, which is "not
    greater", as in the reference.  Host only, NumPy float64."""
    if mode not in MODES:
        raise ValueError('select_views: mode must be one of "val", "w1", "train", "all", got %r' % (mode,))
    if not _is_int(window_size) or window_size < 1:
        raise ValueError("select_views: window_size must be a positive int, got %r" % (window_size,))
    if not _is_num(min_angle) or not _is_num(min_distance):
        raise ValueError("select_views: min_angle and min_distance must be numbers, got %r, %r" % (min_angle, min_distance))
    if isinstance(T_world_camera, dict):
        items = [(k, np.asarray(v, np.float64)) for k, v in T_world_camera.items()]
    else:
        M = np.asarray(raw(T_world_camera).cpu() if isinstance(raw(T_world_camera), torch.Tensor) else T_world_camera, np.float64)
        if M.ndim != 3 or M.shape[1:] != (4, 4):
            raise ValueError("select_views: T_world_camera must be (n, 4, 4) or a dict of (4, 4), got %s" % (M.shape,))
        items = list(enumerate(M))
    for k, v in items:
        if not _is_int(k) or v.shape != (4, 4):
            raise ValueError("select_views: frame %r must be an int id with a (4, 4) pose, got %s" % (k, v.shape))
    poses = {int(k): v for k, v in items if np.all(np.isfinite(v))}
    z = np.array([0.0, 0.0, 1.0])
    limit = (min_angle / 180) * np.pi
    keys, groups, ids, last, last_id = [], [], [], None, 0
    for i, M in poses.items():
        last_id = i
        first = last is None
        if not first:
            with np.errstate(invalid="ignore"):
                angle = np.arccos(((np.linalg.inv(M[:3, :3]) @ last[:3, :3] @ z.T) * z).sum())
            dis = np.linalg.norm(M[:3, 3] - last[:3, 3])
            if not (angle > limit or dis > min_distance):
                continue
        keys.append(i)
        last = M
        if mode == "val":
            ids.append(i)
            # a group closes only on a frame taken for its motion (with window_size 1 never: the reference uses "w1" there), and the
            # next group starts from the NEXT frame, whatever its motion
            if not first and len(ids) == window_size:
                groups.append(ids)
                ids, last = [], None
    if mode == "val":
        return groups
    if mode == "w1":
        return [[i] for i in keys]
    if mode == "all":
        return [keys]
    out = []
    for shift in range(10):
        for j in range(len(keys) - window_size + 1):
            win = keys[j:j + window_size]
            if win[-1] + shift <= last_id:
                win = [i + shift for i in win if i + shift in poses]
                if len(win) == window_size and win not in out:
                    out.append(win)
    return out


# ---- the targets ----------------------------------------------------------------------------------------------------------------
def check_levels(levels, max_level):
    """``levels``: 1..8 pairs (points above, ratio above); ``max_level`` in [0, len(levels)].  ValueError, else two ctypes arrays."""
    if not isinstance(levels, (tuple, list)) or not 1 <= len(levels) <= MAX_LEVELS or not all(
            isinstance(p, (tuple, list)) and len(p) == 2 and _is_int(p[0]) and 0 <= p[0] < 2 ** 31 and _is_num(p[1]) and np.isfinite(p[1])
            for p in levels):
        raise ValueError("SnippetTargets: levels must be 1 to %d pairs (points above: int >= 0, ratio above: number), got %r"
                         % (MAX_LEVELS, levels))
    if not _is_int(max_level) or not 0 <= max_level <= len(levels):
        raise ValueError("SnippetTargets: max_level must be an int in [0, %d], got %r" % (len(levels), max_level))
    n = len(levels)
    return (C.c_int32 * n)(*[int(p[0]) for p in levels]), (C.c_float * n)(*[float(p[1]) for p in levels])


def _intrinsics44(what, K, B):
    """float32 (B, 4, 4) on the CPU from (4, 4), (3, 3), (B, 4, 4) or (B, 3, 3)."""
    K = torch.as_tensor(raw(K)).detach().cpu()
    if not K.dtype.is_floating_point or K.ndim not in (2, 3) or tuple(K.shape[-2:]) not in ((3, 3), (4, 4)) or (K.ndim == 3 and K.shape[0] != B):
        raise ValueError("SnippetTargets: %s must be a floating-point (4, 4), (3, 3) or (B = %d, ...) of those, got %s %s"
                         % (what, B, K.dtype, tuple(K.shape)))
    K = K.to(torch.float32)
    if K.shape[-1] == 3:
        K4 = torch.eye(4, dtype=torch.float32).repeat(K.shape[:-2] + (1, 1))
        K4[..., :3, :3] = K
        K = K4
    return (K.expand(B, 4, 4) if K.ndim == 2 else K).contiguous()


class SnippetTargets:
    """``targets(depth, depth_intrinsics, color_intrinsics, color_size, T_world_camera, obbs, sym)`` -> ``{"obbs_padded": Obb3D,
    "sym", "num_valid"}``: what the reference's annotation pass (generate_scannet_anno_snippet.py) makes of a snippet, for B scenes
    at once and on the device.  ``batch.update(targets(...))`` after ``FramePrep`` gives a complete training batch.

    ``depth`` (B, T, Hd, Wd) uint16 on the GPU, contiguous; ``depth_intrinsics`` / ``color_intrinsics`` (4, 4) or (B, 4, 4) ((3, 3)
    is taken too) — the depth intrinsics are inverted here with ``numpy.linalg.inv`` on the float32 matrix, as the reference does —;
    ``color_size`` (h, w) of the colour image; ``T_world_camera`` (B, T, 4, 4) or a (B, T, 12) ``Pose``, any floating type (float64 is
    honoured); ``obbs`` (B, N, 19) rows of the scene with -1 padding (an ``Obb3D`` or a tensor); ``sym`` (B, S), float32 or int32,
    entry n belonging to box n; ``corners_world`` (B, N, 8, 3): honoured as float64 if given as float64, else the corners are derived
    from the rows.  ``obbs_padded`` is (B, max_box, 19) with the valid rows in their order at the front and -1 behind; ``sym`` is
    compacted the same way at its own width; ``num_valid`` (B,) int32 stays on the device.  ``details=True`` adds ``valid`` (bool),
    ``points_inside``, ``truncation``, ``difficulty`` (B, N) and ``frame_points_inside``, ``frame_truncation`` (B, T, N).

    Two launches on the current stream, nothing synchronises; the small host-side arguments are uploaded with non-blocking copies.
    There is no CPU path: CPU depth is a RuntimeError."""

    def __init__(self, levels=DEFAULT_LEVELS, depth_scale=1000, max_level=3, max_box=100):
        self._counts, self._ratios = check_levels(levels, max_level)
        if not _is_num(depth_scale) or not depth_scale > 0 or not np.isfinite(depth_scale):
            raise ValueError("SnippetTargets: depth_scale must be a number above 0, got %r" % (depth_scale,))
        if not _is_int(max_box) or not 1 <= max_box <= 2 ** 20:
            raise ValueError("SnippetTargets: max_box must be an int in [1, 2^20], got %r" % (max_box,))
        self.levels = tuple((int(p[0]), float(p[1])) for p in levels)
        self.max_level, self.depth_scale, self.max_box = int(max_level), float(depth_scale), int(max_box)

    def check_args(self, depth, depth_intrinsics, color_intrinsics, color_size, T_world_camera, obbs, sym, corners_world):
        """Shapes, dtypes and devices (ValueError) before anything touches the GPU.  Returns (B, T, Hd, Wd, N, S) and the host-side
        float32 (B, 4, 4) inverse depth intrinsics and colour intrinsics."""
        if not isinstance(depth, torch.Tensor) or depth.ndim != 4 or min(depth.shape) < 1:
            raise ValueError("SnippetTargets: depth must be (B, T, Hd, Wd), got %s" % (tuple(getattr(depth, "shape", ())),))
        if depth.dtype != torch.uint16:
            raise ValueError("SnippetTargets: depth must be a uint16 tensor (millimetres as decoded), got %s" % depth.dtype)
        if not depth.is_contiguous():
            raise ValueError("SnippetTargets: depth must be contiguous (a strided view is not copied for you)")
        B, T, Hd, Wd = depth.shape
        if B > MAX_SCENES or T > MAX_FRAMES or max(Hd, Wd) > MAX_SIDE:
            raise ValueError("SnippetTargets: %d scenes of %d frames of %d x %d; at most %d scenes, %d frames, sides of %d"
                             % (B, T, Wd, Hd, MAX_SCENES, MAX_FRAMES, MAX_SIDE))
        if not isinstance(color_size, (tuple, list)) or len(color_size) != 2 or not all(_is_int(v) and 1 <= v <= MAX_SIDE for v in color_size):
            raise ValueError("SnippetTargets: color_size must be (h, w), two ints in [1, %d], got %r" % (MAX_SIDE, color_size))
        Kd = _intrinsics44("depth_intrinsics", depth_intrinsics, B)
        Kc = _intrinsics44("color_intrinsics", color_intrinsics, B)
        try:
            Ki = np.stack([np.linalg.inv(k) for k in Kd.numpy()])
        except np.linalg.LinAlgError:
            raise ValueError("SnippetTargets: depth_intrinsics is singular") from None
        M = raw(T_world_camera)
        if not isinstance(M, torch.Tensor):
            M = torch.as_tensor(M)
        if tuple(M.shape) not in ((B, T, 4, 4), (B, T, 12)) or not M.dtype.is_floating_point:
            raise ValueError("SnippetTargets: T_world_camera must be a floating-point (B, T, 4, 4) = %s (or a (B, T, 12) Pose), got %s"
                             % ((B, T, 4, 4), tuple(M.shape)))
        rows = raw(obbs)
        if not isinstance(rows, torch.Tensor) or rows.ndim != 3 or rows.shape[0] != B or rows.shape[2] != 19 or rows.shape[1] < 1 \
                or rows.dtype != torch.float32:
            raise ValueError("SnippetTargets: obbs must be float32 (B = %d, N >= 1, 19), got %s %s"
                             % (B, getattr(rows, "dtype", type(rows)), tuple(getattr(rows, "shape", ()))))
        N = rows.shape[1]
        if N > MAX_BOXES:
            raise ValueError("SnippetTargets: %d boxes per scene; at most %d" % (N, MAX_BOXES))
        if not isinstance(sym, torch.Tensor) or sym.ndim != 2 or sym.shape[0] != B or sym.shape[1] < 1 or sym.shape[1] > 2 ** 20 \
                or sym.dtype not in (torch.float32, torch.int32):
            raise ValueError("SnippetTargets: sym must be float32 or int32 (B = %d, S >= 1), got %s %s"
                             % (B, getattr(sym, "dtype", type(sym)), tuple(getattr(sym, "shape", ()))))
        if corners_world is not None:
            if not isinstance(corners_world, torch.Tensor) or tuple(corners_world.shape) != (B, N, 8, 3) or not corners_world.dtype.is_floating_point:
                raise ValueError("SnippetTargets: corners_world must be a floating-point (B, N, 8, 3) = %s, got %s"
                                 % ((B, N, 8, 3), tuple(getattr(corners_world, "shape", ()))))
        return (B, T, Hd, Wd, N, sym.shape[1]), torch.from_numpy(Ki), Kc

    @torch.no_grad()
    def __call__(self, depth, depth_intrinsics, color_intrinsics, color_size, T_world_camera, obbs, sym, corners_world=None, details=False):
        from . import _lib
        (B, T, Hd, Wd, N, S), Ki, Kc = self.check_args(depth, depth_intrinsics, color_intrinsics, color_size, T_world_camera, obbs, sym,
                                                       corners_world)
        if not depth.is_cuda:
            raise RuntimeError("parq_amd.SnippetTargets: the depth is on %s; the targets are made on the GPU only (there is no CPU "
                               "fallback)" % depth.device)
        lib = _lib.load()
        dev = depth.device
        dp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(dev):
            Ki, Kc = Ki.to(dev, non_blocking=True), Kc.to(dev, non_blocking=True)
            M = raw(T_world_camera)
            M = (M if isinstance(M, torch.Tensor) else torch.as_tensor(M)).detach().to(dev, non_blocking=True).to(torch.float64)
            if M.shape[-1] != 12:
                M = torch.cat([M[..., :3, :3].reshape(B, T, 9), M[..., :3, 3]], dim=-1)
            M = M.contiguous()
            rows = raw(obbs).detach().to(dev, non_blocking=True).contiguous()
            sym_d = sym.detach().to(dev, non_blocking=True).contiguous()
            corners = None
            if corners_world is not None and corners_world.dtype == torch.float64:
                corners = corners_world.detach().to(dev, non_blocking=True).contiguous()
            need = lib.parq_snippet_targets_workspace(B, T, Hd, Wd, N)
            if need == 0:
                raise RuntimeError("parq_amd: parq_snippet_targets_workspace refused B = %d, T = %d, %d x %d, N = %d" % (B, T, Wd, Hd, N))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            out_rows = torch.empty(B, self.max_box, 19, dtype=torch.float32, device=dev)
            out_sym = torch.empty(B, S, dtype=sym_d.dtype, device=dev)
            num = torch.empty(B, dtype=torch.int32, device=dev)
            fp = torch.empty(B, T, N, dtype=torch.int32, device=dev)
            ft = torch.empty(B, T, N, dtype=torch.float32, device=dev)
            pts = torch.empty(B, N, dtype=torch.int32, device=dev)
            tr = torch.empty(B, N, dtype=torch.float32, device=dev)
            diff = torch.empty(B, N, dtype=torch.int32, device=dev)
            valid = torch.empty(B, N, dtype=torch.int32, device=dev)
            _lib.check(lib.parq_snippet_targets(dp(depth.detach()), B, T, Hd, Wd, dp(Ki), dp(Kc), int(color_size[0]), int(color_size[1]),
                                                dp(M), dp(rows), dp(corners), dp(sym_d), int(sym_d.dtype == torch.int32), S, N, self.max_box,
                                                self._counts, self._ratios, len(self.levels), self.max_level, self.depth_scale, dp(ws),
                                                need, dp(out_rows), dp(out_sym), dp(num), dp(fp), dp(ft), dp(pts), dp(tr), dp(diff),
                                                dp(valid), _lib.stream_ptr()), "parq_snippet_targets")
            res = {"obbs_padded": Obb3D(out_rows), "sym": out_sym, "num_valid": num}
            if details:
                res.update(valid=valid != 0, points_inside=pts, truncation=tr, difficulty=diff, frame_points_inside=fp, frame_truncation=ft)
        return res
