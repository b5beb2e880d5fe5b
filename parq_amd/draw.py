"""Predicted / ground-truth boxes drawn into the input views on the device (include/parq_hip.h parq_draw_boxes, csrc/draw.hip).

The reference draws with cv2 in a host loop over views x boxes (utils/parq_utils.py:141-211 ``draw_detections``), several
``.cpu()`` round trips per box.  Here the images, cameras, poses and world-frame box corners stay where they are: one min / max
launch, one projection launch and one image-sized raster launch write the ``(B, 3, T*H, W)`` overlays with no host round trip.

The drawing rule is this project's own (INTEGRATION.md "Drawing detections"); pixel equality with OpenCV's ``line`` is not
claimed.  Per view the image is normalised ``(x - min) / (max - min)`` in float32 (NaN propagates as in NumPy); the 8 corners
of a box are projected in float64 in a fixed operation order, a corner is valid in front of the 1e-3 plane and inside the
camera's image, and each of the 12 edges with two valid corners is drawn between the truncated integer endpoints as a capsule
of half-width 1 px evaluated in integers.  Boxes are drawn in index order, later over earlier.
"""
from __future__ import annotations

import colorsys
import ctypes as C
from fractions import Fraction

import numpy as np
import torch

from .wrappers import raw

OUT_DTYPES = (torch.float32, torch.uint8)
MAX_SIDE = 8192                     # H, W beyond this are refused by the library (the integer capsule test is sized for it)

_color_cache = {}


def _hues():
    """0, 1/2, 1/4, 3/4, 1/8, 3/8, ...: every odd numerator over each power of two in turn."""
    yield Fraction(0)
    den = 2
    while True:
        for num in range(1, den, 2):
            yield Fraction(num, den)
        den *= 2


def box_colors(num_semcls):
    """float32 ``(num_semcls, 3)``: the class colours of the reference's ``get_colors(num_semcls)`` — saturation 0.6, each hue
    of the sequence above first at value 0.6, then at value 0.9."""
    if isinstance(num_semcls, bool) or not isinstance(num_semcls, int) or num_semcls < 0:
        raise ValueError("box_colors: num_semcls must be a non-negative int, got %r" % (num_semcls,))
    sat, values = Fraction(6, 10), (Fraction(6, 10), Fraction(9, 10))
    rows = []
    for hue in _hues():
        for val in values:
            if len(rows) == num_semcls:
                return np.asarray(rows, dtype=np.float32).reshape(num_semcls, 3)
            rows.append([float(ch) for ch in colorsys.hsv_to_rgb(hue, sat, val)])


def check_draw_args(images, camera, T_camera_pseudoCam, T_world_pseudoCam, corners_world, labels, keep, count, num_semcls, dtype, out):
    """Shapes, dtypes and devices of a ``draw_boxes`` call (ValueError), before anything touches the GPU.  Returns the raw
    tensors and ``(B, T, H, W, M)``."""
    img, cam, T_cp, T_wp, cw, lab = (raw(a) for a in (images, camera, T_camera_pseudoCam, T_world_pseudoCam, corners_world, labels))
    keep = None if keep is None else raw(keep)
    count = None if count is None else raw(count)
    if isinstance(num_semcls, bool) or not isinstance(num_semcls, int) or num_semcls < 1:
        raise ValueError("draw_boxes: num_semcls must be a positive int, got %r" % (num_semcls,))
    if dtype not in OUT_DTYPES:
        raise ValueError("draw_boxes: dtype must be torch.float32 or torch.uint8, got %r" % (dtype,))
    if not isinstance(img, torch.Tensor) or img.ndim != 5 or img.shape[2] != 3 or min(img.shape) < 1:
        raise ValueError("draw_boxes: images must be (B, T, 3, H, W), got %s" % (tuple(getattr(img, "shape", ())),))
    if img.dtype != torch.float32:
        raise ValueError("draw_boxes: images must be a float32 tensor, got %s" % img.dtype)
    B, T, _, H, W = img.shape
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError("draw_boxes: images of %d x %d; at most %d x %d" % (H, W, MAX_SIDE, MAX_SIDE))
    for name, t, width in (("camera", cam, 6), ("T_camera_pseudoCam", T_cp, 12), ("T_world_pseudoCam", T_wp, 12)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, T, width):
            raise ValueError("draw_boxes: %s must be (B, T, %d) = %s, got %s" % (name, width, (B, T, width), tuple(getattr(t, "shape", ()))))
        if not t.dtype.is_floating_point:
            raise ValueError("draw_boxes: %s must be a floating-point tensor, got %s" % (name, t.dtype))
    if not isinstance(cw, torch.Tensor) or cw.ndim != 4 or cw.shape[0] != B or tuple(cw.shape[2:]) != (8, 3):
        raise ValueError("draw_boxes: corners_world must be (B, M, 8, 3) with B = %d, got %s" % (B, tuple(getattr(cw, "shape", ()))))
    if not cw.dtype.is_floating_point:
        raise ValueError("draw_boxes: corners_world must be a floating-point tensor, got %s" % cw.dtype)
    M = cw.shape[1]
    if not isinstance(lab, torch.Tensor) or tuple(lab.shape) != (B, M):
        raise ValueError("draw_boxes: labels must be (B, M) = %s, got %s" % ((B, M), tuple(getattr(lab, "shape", ()))))
    if lab.dtype.is_floating_point or lab.dtype.is_complex or lab.dtype == torch.bool:
        raise ValueError("draw_boxes: labels must be an integer tensor, got %s" % lab.dtype)
    if keep is not None:
        if not isinstance(keep, torch.Tensor) or tuple(keep.shape) != (B, M):
            raise ValueError("draw_boxes: keep must be (B, M) = %s, got %s" % ((B, M), tuple(getattr(keep, "shape", ()))))
        if keep.dtype not in (torch.bool, torch.uint8):
            raise ValueError("draw_boxes: keep must be a bool or uint8 tensor, got %s" % keep.dtype)
    if count is not None:
        if not isinstance(count, torch.Tensor) or tuple(count.shape) != (B,):
            raise ValueError("draw_boxes: count must be (B,) = %s, got %s" % ((B,), tuple(getattr(count, "shape", ()))))
        if count.dtype.is_floating_point or count.dtype.is_complex or count.dtype == torch.bool:
            raise ValueError("draw_boxes: count must be an integer tensor, got %s" % count.dtype)
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, 3, T * H, W) or out.dtype != dtype or not out.is_contiguous():
            raise ValueError("draw_boxes: out must be a contiguous %s tensor of %s, got %s %s"
                             % (dtype, (B, 3, T * H, W), getattr(out, "dtype", type(out)), tuple(getattr(out, "shape", ()))))
    for name, t in (("camera", cam), ("T_camera_pseudoCam", T_cp), ("T_world_pseudoCam", T_wp), ("corners_world", cw), ("labels", lab),
                    ("keep", keep), ("count", count), ("out", out)):
        if t is not None and t.device != img.device:
            raise ValueError("draw_boxes: %s is on %s, the images on %s (a tensor is not moved for you)" % (name, t.device, img.device))
    return (img, cam, T_cp, T_wp, cw, lab, keep, count), (B, T, H, W, M)


def _colors_on(device, num_semcls):
    key = (device, num_semcls)
    if key not in _color_cache:
        _color_cache[key] = torch.from_numpy(box_colors(num_semcls)).to(device)
    return _color_cache[key]


@torch.no_grad()
def draw_boxes(images, camera, T_camera_pseudoCam, T_world_pseudoCam, corners_world, labels, keep=None, count=None, *, num_semcls,
               dtype=torch.float32, out=None):
    """``(B, 3, T*H, W)``: the views of every scene normalised per view, stacked vertically, with the boxes' edges drawn in their
    class colours (``box_colors(num_semcls)``; label ``num_semcls`` is the background and is not drawn).

    ``images`` (B,T,3,H,W) float32; ``camera`` (B,T,6), ``T_camera_pseudoCam`` / ``T_world_pseudoCam`` (B,T,12): this project's
    wrappers or raw tensors; ``corners_world`` (B,M,8,3) in ``Obb3D.bb3corners_object`` order; ``labels`` (B,M) integers;
    ``keep`` (B,M) bool or None; ``count`` (B,) integers or None: only boxes ``m < count[b]`` of scene ``b`` (padded ground
    truth).  ``dtype``: ``torch.float32``, or ``torch.uint8`` for ``trunc(value * 255)`` (NaN gives 0).  Enqueues three
    launches on the current stream and does not synchronise.  There is no CPU path: CPU tensors are a RuntimeError."""
    from . import _lib
    (img, cam, T_cp, T_wp, cw, lab, keep, count), (B, T, H, W, M) = check_draw_args(
        images, camera, T_camera_pseudoCam, T_world_pseudoCam, corners_world, labels, keep, count, num_semcls, dtype, out)
    if not img.is_cuda:
        raise RuntimeError("parq_amd.draw_boxes: the images are on %s; drawing runs on the GPU only (there is no CPU fallback)" % img.device)
    lib = _lib.load()
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    img, cam, T_cp, T_wp, cw = f32(img), f32(cam), f32(T_cp), f32(T_wp), f32(cw)
    lab = lab.to(torch.int32).contiguous()
    keep = None if keep is None else keep.contiguous().view(torch.uint8)         # a bool tensor is one byte per element as it is
    count = None if count is None else count.to(torch.int32).contiguous()
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    with torch.cuda.device(img.device):
        colors = _colors_on(img.device, num_semcls)
        nbytes = lib.parq_draw_boxes_workspace_bytes(B, T, M)
        if nbytes == 0:
            raise ValueError("draw_boxes: B * T = %d views, M = %d boxes are more than one call takes (65535 views, 2^24 boxes)" % (B * T, M))
        ws = torch.empty((nbytes + 15) // 16 * 2, dtype=torch.float64, device=img.device)
        if out is None:
            out = torch.empty(B, 3, T * H, W, dtype=dtype, device=img.device)
        _lib.check(lib.parq_draw_boxes(dp(img), dp(cam), dp(T_cp), dp(T_wp), dp(cw), dp(lab), dp(keep), dp(count), dp(colors),
                                       num_semcls + 1, B, T, H, W, M, dp(ws), ws.numel() * 8, dp(out), int(dtype == torch.uint8),
                                       _lib.stream_ptr()), "parq_draw_boxes")
    return out
