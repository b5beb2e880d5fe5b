"""Raw camera frames prepared on the device: resize, intrinsics, poses (include/parq_hip.h parq_frames_resize, csrc/frames.hip).

The reference prepares every snippet on the host (datasets/transforms.py:211-237 ``ScanNetBaseTransform``): ``pad_scannet`` +
``ResizeImage`` through Pillow on one core (3.5 ms per 1296 x 972 frame on the MI355X box's host), ``ToTensor``, ``Normalize``, ``Convert2Objects``,
``GravityAligned`` and ``SnippetLocal``.  Here decoded ``uint8`` frames in GPU memory go through one launch that restates Pillow's
8-bit bilinear resample in integers — every byte equal — and the camera and pose keys are a handful of small tensor operations:

    resize_frames       pad_scannet + ResizeImage + ToTensor + Normalize   (..., H, W, 3) uint8 -> (..., 3, h, w)
    resized_intrinsics  the intrinsics arithmetic of pad_scannet + ResizeImage, in float64
    gravity_aligned     GravityAligned                                      T_world_camera -> T_world_pseudoCam, T_camera_pseudoCam
    snippet_local       SnippetLocal                                        T_world_pseudoCam -> T_world_local
    FramePrep           all of it: the batch ``PARQ.forward`` reads when a ``backbone2d`` is plugged in

JPEG decoding stays the caller's, and so does the ResNet body of the backbone.  The resize rule is stated in full in
include/parq_hip.h and INTEGRATION.md "From raw frames".
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .wrappers import Camera, Pose, raw

OUT_DTYPES = (torch.float32, torch.uint8)
MAX_SIDE = 8192            # every side — input, padded input, output — beyond this is refused by the library
MAX_DOWNSCALE = 8          # padded input side <= MAX_DOWNSCALE * output side (17 taps); upscaling is not limited
MAX_FRAMES = 65535         # frames of one call
SCANNET_SIZE = (1296, 968)          # the (W, H) the reference's pad_scannet pads by 2 rows at the top and at the bottom
SCANNET_PAD = (0, 2, 0, 2)

_plan_cache = {}
_up_cache = {}


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_size_pad(what, in_size, size, pad):
    """``size`` (width, height), ``pad`` "scannet" / None / (left, top, right, bottom) for frames of ``in_size`` (W, H): ValueError,
    else ``(w, h), (left, top, right, bottom)`` as ints."""
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(_is_int(v) and v >= 1 for v in size):
        raise ValueError("%s: size must be (width, height), two positive ints, got %r" % (what, size))
    if not isinstance(in_size, (tuple, list)) or len(in_size) != 2 or not all(_is_int(v) and v >= 1 for v in in_size):
        raise ValueError("%s: in_size must be (width, height), two positive ints, got %r" % (what, in_size))
    W, H = (int(v) for v in in_size)
    if pad is None:
        pad4 = (0, 0, 0, 0)
    elif isinstance(pad, str):
        if pad != "scannet":
            raise ValueError('%s: pad must be "scannet", None or (left, top, right, bottom), got %r' % (what, pad))
        pad4 = SCANNET_PAD if (W, H) == SCANNET_SIZE else (0, 0, 0, 0)
    elif isinstance(pad, (tuple, list)) and len(pad) == 4 and all(_is_int(v) and v >= 0 for v in pad):
        pad4 = tuple(int(v) for v in pad)
    else:
        raise ValueError('%s: pad must be "scannet", None or (left, top, right, bottom) of non-negative ints, got %r' % (what, pad))
    w, h = (int(v) for v in size)
    Wp, Hp = W + pad4[0] + pad4[2], H + pad4[1] + pad4[3]
    if max(W, H, Wp, Hp, w, h) > MAX_SIDE:
        raise ValueError("%s: frames of %d x %d (padded %d x %d) to %d x %d; every side at most %d" % (what, W, H, Wp, Hp, w, h, MAX_SIDE))
    if Wp > MAX_DOWNSCALE * w or Hp > MAX_DOWNSCALE * h:
        raise ValueError("%s: %d x %d (padded) to %d x %d shrinks a side more than %d times" % (what, Wp, Hp, w, h, MAX_DOWNSCALE))
    return (w, h), pad4


def check_frames_args(frames, size, pad, dtype, out):
    """Shapes, dtypes and devices of a ``resize_frames`` call (ValueError), before anything touches the GPU.  Returns
    ``lead, (H, W), (w, h), pad4``: the leading shape, the frame size, the output size and the border."""
    if dtype not in OUT_DTYPES:
        raise ValueError("resize_frames: dtype must be torch.float32 or torch.uint8, got %r" % (dtype,))
    if not isinstance(frames, torch.Tensor) or frames.ndim < 3 or frames.shape[-1] != 3 or min(frames.shape) < 1:
        raise ValueError("resize_frames: frames must be (..., H, W, 3) with at least one frame, got %s" % (tuple(getattr(frames, "shape", ())),))
    if frames.dtype != torch.uint8:
        raise ValueError("resize_frames: frames must be a uint8 tensor (decoded RGB bytes), got %s" % frames.dtype)
    if not frames.is_contiguous():
        raise ValueError("resize_frames: frames must be contiguous (rows of 3 * W bytes; a strided view is not copied for you)")
    lead, (H, W) = tuple(frames.shape[:-3]), frames.shape[-3:-1]
    (w, h), pad4 = check_size_pad("resize_frames", (W, H), size, pad)
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if n > MAX_FRAMES:
        raise ValueError("resize_frames: %d frames in one call; at most %d" % (n, MAX_FRAMES))
    if out is not None:
        want = lead + (3, h, w)
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != want or out.dtype != dtype or not out.is_contiguous():
            raise ValueError("resize_frames: out must be a contiguous %s tensor of %s, got %s %s"
                             % (dtype, want, getattr(out, "dtype", type(out)), tuple(getattr(out, "shape", ()))))
        if out.device != frames.device:
            raise ValueError("resize_frames: out is on %s, the frames on %s" % (out.device, frames.device))
    return lead, (H, W), (w, h), pad4


def frame_plan(in_size, out_size):
    """int32 NumPy array: the plan of one axis as ``parq_frame_plan`` writes it — ``[ksize, (xmin, n, k[0..ksize)) per output]``."""
    from . import _lib
    lib = _lib.load()
    n = lib.parq_frame_plan_ints(in_size, out_size)
    if n == 0:
        raise ValueError("frame_plan: %d -> %d: sizes from 1 to %d, at most %d times smaller" % (in_size, out_size, MAX_SIDE, MAX_DOWNSCALE))
    plan = np.zeros(n, np.int32)
    rc = lib.parq_frame_plan(in_size, out_size, plan.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise RuntimeError("parq_amd: parq_frame_plan(%d, %d) failed (code %d)" % (in_size, out_size, rc))
    return plan


def _plan_on(device, in_size, out_size):
    key = (device, in_size, out_size)
    if key not in _plan_cache:
        _plan_cache[key] = torch.from_numpy(frame_plan(in_size, out_size)).to(device)
    return _plan_cache[key]


@torch.no_grad()
def resize_frames(frames, size=(320, 240), pad="scannet", dtype=torch.float32, out=None):
    """``(..., 3, h, w)``: every ``(H, W, 3)`` uint8 frame zero-padded by ``pad`` and resized to ``size = (width, height)`` exactly
    as Pillow's ``Image.resize(size, Image.BILINEAR)`` does it, channels first.  ``dtype=torch.float32``: bytes / 255 (one correctly
    rounded division: what ``ResizeImage`` + ``ToTensor`` + ``Normalize`` give); ``torch.uint8``: the bytes.

    ``pad``: ``"scannet"`` — (0, 2, 0, 2) for 1296 x 968 frames, nothing otherwise (the reference's ``pad_scannet``) —, ``None``, or
    ``(left, top, right, bottom)``.  One launch on the current stream, no synchronisation; the two axis plans are made on the host
    and uploaded once per (device, sizes).  There is no CPU path: CPU tensors are a RuntimeError."""
    from . import _lib
    lead, (H, W), (w, h), pad4 = check_frames_args(frames, size, pad, dtype, out)
    if not frames.is_cuda:
        raise RuntimeError("parq_amd.resize_frames: the frames are on %s; the resize runs on the GPU only (there is no CPU fallback)"
                           % frames.device)
    lib = _lib.load()
    n = int(np.prod(lead, dtype=np.int64)) if lead else 1
    dp = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(frames.device):
        plan_x = _plan_on(frames.device, W + pad4[0] + pad4[2], w)
        plan_y = _plan_on(frames.device, H + pad4[1] + pad4[3], h)
        if out is None:
            out = torch.empty(lead + (3, h, w), dtype=dtype, device=frames.device)
        _lib.check(lib.parq_frames_resize(dp(frames.detach()), n, H, W, pad4[0], pad4[1], pad4[2], pad4[3], dp(plan_x), dp(plan_y), h, w,
                                          dp(out), int(dtype == torch.uint8), _lib.stream_ptr()), "parq_frames_resize")
    return out


def resized_intrinsics(K, in_size, size, pad):
    """float32 ``(..., 3, 3)``: the intrinsics after ``pad`` and the resize of ``in_size = (W, H)`` frames to ``size = (w, h)``, by the
    reference's arithmetic in float64 (datasets/transforms.py:73,92-93): ``cx += left``, ``cy += top``, row 0 ``/= Wp / w``, row 1
    ``/= Hp / h``; cast to float32 at the end, as ``ToTensor`` does.  ``K``: a tensor or array ``(..., 3, 3)``; stays on its device."""
    (w, h), pad4 = check_size_pad("resized_intrinsics", tuple(in_size), size, pad)
    K = torch.as_tensor(K)
    if K.ndim < 2 or tuple(K.shape[-2:]) != (3, 3) or not K.dtype.is_floating_point:
        raise ValueError("resized_intrinsics: K must be a floating-point (..., 3, 3), got %s %s" % (K.dtype, tuple(K.shape)))
    Wp, Hp = in_size[0] + pad4[0] + pad4[2], in_size[1] + pad4[1] + pad4[3]
    K = K.detach().to(torch.float64).clone()
    K[..., 0, 2] += pad4[0]
    K[..., 1, 2] += pad4[1]
    K[..., 0, :] /= Wp / w
    K[..., 1, :] /= Hp / h
    return K.to(torch.float32)


def _unit_or_same(v):
    """v / |v| where |v| is not 0, v where it is — per vector, without asking the device (the reference's ``normalize`` returns
    EVERY vector of the batch as it is as soon as one has norm 0, which needs a host round trip and lets one view decide for all)."""
    norm = torch.norm(v, dim=-1, keepdim=True)
    return torch.where(norm == 0, v, v / norm)


def _up_on(device, up):
    """``up`` and ``up / |up|`` as float32 tensors on ``device``, uploaded once (an upload per call would stall the host)."""
    key = (device, up)
    if key not in _up_cache:
        up_w = torch.tensor(up, dtype=torch.float32)
        _up_cache[key] = (up_w.to(device), (up_w / torch.norm(up_w, dim=-1, keepdim=True)).to(device))
    return _up_cache[key]


@torch.no_grad()
def gravity_aligned(T_world_camera, up=(0, 0, 1)):
    """``(T_world_pseudoCam, T_camera_pseudoCam)`` as ``Pose``: the gravity-aligned frame of every camera (the reference's
    ``GravityAligned``, datasets/transforms.py:22-62, in its order of float32 operations): column 1 of the rotation is ``up``,
    column 2 the normalised rejection of the camera's forward axis from ``up``, column 0 the normalised ``cross(col1, col2)``, the
    translation the camera's; ``T_camera_pseudoCam = T_world_camera.inverse() @ T_world_pseudoCam``.

    ``T_world_camera``: ``(..., 4, 4)`` matrices or a ``Pose``.  One deliberate difference: a vector is normalised wherever ITS norm
    is not 0; the reference skips the normalisation of every view as soon as one view's norm is 0 (a camera looking straight along
    ``up``).  The two agree whenever no view does.  No host synchronisation."""
    if not isinstance(up, (tuple, list)) or len(up) != 3 or not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in up) \
            or not any(up):
        raise ValueError("gravity_aligned: up must be three numbers, not all 0, got %r" % (up,))
    if isinstance(T_world_camera, Pose):
        T_wc = Pose(T_world_camera._data.detach().float())
    else:
        M = torch.as_tensor(T_world_camera)
        if M.ndim < 2 or tuple(M.shape[-2:]) != (4, 4) or not M.dtype.is_floating_point:
            raise ValueError("gravity_aligned: T_world_camera must be a floating-point (..., 4, 4) or a Pose, got %s" % (tuple(M.shape),))
        T_wc = Pose.from_4x4mat(M.detach().float())
    R_wc = T_wc.R
    up_w, unit_up = _up_on(R_wc.device, tuple(float(v) for v in up))
    forward = R_wc[..., :, 2]
    project = (forward.unsqueeze(-2) @ unit_up.unsqueeze(-1)).squeeze(-1) * unit_up
    R_wp = torch.zeros_like(R_wc)
    R_wp[..., 1] = up_w
    R_wp[..., 2] = _unit_or_same(forward - project)
    R_wp[..., 0] = _unit_or_same(torch.cross(R_wp[..., 1], R_wp[..., 2], dim=-1))
    T_wp = Pose.from_Rt(R_wp, T_wc.t.clone())
    return T_wp, T_wc.inverse() @ T_wp


def snippet_local(T_world_pseudoCam, frame_selection=0.5):
    """``(B, 1, 12)``: the pose of view ``int(T * frame_selection)`` of every scene's ``(B, T, 12)`` poses — the snippet's local frame
    (the reference's ``SnippetLocal``).  A ``Pose`` gives a ``Pose``, a tensor a tensor; the result is a copy."""
    d = raw(T_world_pseudoCam)
    if not isinstance(d, torch.Tensor) or d.ndim != 3 or d.shape[-1] != 12 or d.shape[1] < 1:
        raise ValueError("snippet_local: T_world_pseudoCam must be (B, T, 12), got %s" % (tuple(getattr(d, "shape", ())),))
    if isinstance(frame_selection, bool) or not isinstance(frame_selection, (int, float)) or not 0 <= frame_selection < 1:
        raise ValueError("snippet_local: frame_selection must be a number in [0, 1), got %r" % (frame_selection,))
    t = int(d.shape[1] * frame_selection)
    local = d[:, t:t + 1].detach().clone()
    return Pose(local) if isinstance(T_world_pseudoCam, Pose) else local


class FramePrep:
    """``prep(frames, intrinsics, T_world_camera)`` -> the batch keys ``PARQ.forward`` reads in front of a ``backbone2d``: what the
    reference's ``ScanNetBaseTransform`` (datasets/transforms.py:211-237) makes of a snippet, for B scenes at once and on the device.

    ``frames`` (B, T, H, W, 3) uint8 on the GPU; ``intrinsics`` (B, T, 3, 3) of the frames as they are, before pad and resize;
    ``T_world_camera`` (B, T, 4, 4).  The two small tensors are moved to the frames' device if they are elsewhere.  The result:
    ``rgb_img`` (B, T, 3, h, w) float32 in [0, 1]; ``camera`` a ``Camera`` of ``[w, h, fx, fy, cx, cy]`` — as in ``Convert2Objects`` the
    intrinsics of view 0 of each scene for all its views (``first_view_intrinsics=False``: each view's own) —; ``T_world_camera``,
    ``T_world_pseudoCam``, ``T_camera_pseudoCam`` (B, T, 12) and ``T_world_local`` (B, 1, 12) as ``Pose``."""

    def __init__(self, size=(320, 240), pad="scannet", up=(0, 0, 1), frame_selection=0.5, first_view_intrinsics=True):
        check_size_pad("FramePrep", (1, 1), size, None)
        if pad is not None:
            check_size_pad("FramePrep", tuple(size), size, pad)          # the kind of `pad`; its fit to the frames is checked per call
        self.size = (int(size[0]), int(size[1]))
        self.pad = pad
        self.up = tuple(up) if isinstance(up, (tuple, list)) else up
        gravity_aligned(torch.eye(4), self.up)
        snippet_local(torch.zeros(1, 1, 12), frame_selection)
        self.frame_selection = frame_selection
        self.first_view_intrinsics = bool(first_view_intrinsics)

    def __call__(self, frames, intrinsics, T_world_camera):
        if not isinstance(frames, torch.Tensor) or frames.ndim != 5:
            raise ValueError("FramePrep: frames must be (B, T, H, W, 3), got %s" % (tuple(getattr(frames, "shape", ())),))
        lead, (H, W), (w, h), _ = check_frames_args(frames, self.size, self.pad, torch.float32, None)
        B, T = lead
        K, M = torch.as_tensor(intrinsics), raw(T_world_camera)
        M = torch.as_tensor(M)
        if tuple(K.shape) != (B, T, 3, 3) or not K.dtype.is_floating_point:
            raise ValueError("FramePrep: intrinsics must be a floating-point (B, T, 3, 3) = %s, got %s" % ((B, T, 3, 3), tuple(K.shape)))
        if tuple(M.shape) not in ((B, T, 4, 4), (B, T, 12)) or not M.dtype.is_floating_point:
            raise ValueError("FramePrep: T_world_camera must be a floating-point (B, T, 4, 4) = %s (or a (B, T, 12) Pose), got %s"
                             % ((B, T, 4, 4), tuple(M.shape)))
        rgb = resize_frames(frames, self.size, self.pad, torch.float32)
        dev = frames.device
        K = resized_intrinsics(K.to(dev), (W, H), self.size, self.pad)
        if self.first_view_intrinsics:
            K = K[:, :1].expand(B, T, 3, 3)
        cam = torch.stack([K.new_full((B, T), float(w)), K.new_full((B, T), float(h)), K[..., 0, 0], K[..., 1, 1], K[..., 0, 2],
                           K[..., 1, 2]], dim=-1)
        T_wc = Pose(M.to(dev).float()) if M.shape[-1] == 12 else Pose.from_4x4mat(M.to(dev).float())
        T_wp, T_cp = gravity_aligned(T_wc, self.up)
        return {"rgb_img": rgb, "camera": Camera(cam), "T_world_camera": T_wc, "T_world_pseudoCam": T_wp, "T_camera_pseudoCam": T_cp,
                "T_world_local": snippet_local(T_wp, self.frame_selection)}
