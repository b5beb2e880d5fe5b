"""AddRayPE: host-side mirror of model/ray_positional_encoding.py:29-139 on the HIP path.

Same constructor arguments, same ``encoder.{0,2}`` state_dict keys, same ``forward`` signature
and result (the encoding, shaped (B, T, C, H, W)) as the reference module.  The arithmetic runs in
libparq_hip.so (``parq_ray_pe``); ``tokens()`` is the fused fast path that adds the feature maps
and returns the channels-last token tensor the decoder consumes, skipping the NCHW round trip of
model/parq_lightning.py:72-85.
"""
from __future__ import annotations

import ctypes as C
import weakref

import torch
from torch import nn

from . import _lib
from .wrappers import raw


def _node_forward(ctx, mod, out_dims):
    """What both autograd nodes keep of their forward: the module, the dims and geometry, and the workspace holding the hidden layer."""
    ctx.mod, ctx.dims = mod, out_dims
    ctx.geo = mod._last_geo
    # the node owns the workspace of its forward (the hidden layer the backward reads): a later call, while this node is
    # alive and has not run its backward, takes a workspace of its own (several outstanding forwards per module)
    ctx.hold = _WsHold(mod._ws, mod._gen)
    mod._ws_owner = weakref.ref(ctx.hold)


def _encoder_backward(ctx, g, dfeat):
    """parq_ray_pe_backward_flags for the node of ``ctx``: the four encoder gradients (and d features into ``dfeat`` if given),
    fixed-order under torch.use_deterministic_algorithms(True), averaged over the ranks with ``dp_all_reduce``."""
    mod = ctx.mod
    hold = ctx.hold
    if getattr(hold.ws, "_parq_gen", None) != hold.gen:
        raise RuntimeError("parq_amd.AddRayPE: second backward (retain_graph=True) through a tokens() call whose workspace was "
                           "released by the first backward and has since been reused by a later call of the same module")
    B, V, h, w = ctx.dims
    Cd, S = mod.dim_out, mod.num_samples
    cam, T_cp, T_wp, T_wl = ctx.geo
    dev = cam.device
    lib = _lib.load()
    # torch.use_deterministic_algorithms(True): the weight / bias gradients sum their row-range partials in a fixed order
    flags = 1 if torch.are_deterministic_algorithms_enabled() else 0         # PARQ_RAYPE_BWD_DETERMINISTIC
    nbytes = lib.parq_ray_pe_backward_workspace_bytes_flags(B, V, h, w, Cd, S, flags)
    bws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=dev)
    # the four parameter gradients live in ONE flat buffer, so data-parallel training averages them with a single
    # collective (train.py:103: DDP reduces every trainable parameter of the module, the encoder MLP included)
    sizes = (Cd * 3 * S, Cd, Cd * Cd, Cd)
    flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
    dw1, db1, dw2, db2 = (t.view(shape) for t, shape in zip(flat.split(sizes), ((Cd, 3 * S), (Cd,), (Cd, Cd), (Cd,))))
    w2 = mod.encoder[2].weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    _lib.check(lib.parq_ray_pe_backward_flags(_lib.ptr(cam), _lib.ptr(T_cp), _lib.ptr(T_wp), _lib.ptr(T_wl), _lib.ptr(w2),
                                              (C.c_float * 6)(*mod.ray_points_scale), mod.min_depth, mod.max_depth, S, B, V, h, w, Cd,
                                              _lib.ptr(g), _lib.ptr(hold.ws), _lib.ptr(bws), bws.numel() * 4, _lib.ptr(dw1),
                                              _lib.ptr(db1), _lib.ptr(dw2), _lib.ptr(db2), _lib.ptr(dfeat), flags, _lib.stream_ptr()),
               "parq_ray_pe_backward_flags")
    hold.consumed = True
    if mod.dp_all_reduce:
        from .parallel import all_reduce_mean_
        all_reduce_mean_(flat)
    return dw1, db1, dw2, db2


class _RayPeFn(torch.autograd.Function):
    """tokens = features + encoding as one autograd node: backward = parq_ray_pe_backward (gradients of the encoder MLP and
    of the feature maps; the ray geometry has no learnable part)."""

    @staticmethod
    def forward(ctx, mod, features, camera, T_cp, T_wp, T_wl, w1, b1, w2, b2):
        out, dims, _ = mod._run(camera, T_cp, T_wp, T_wl, tuple(features.shape[-2:]), features, own_workspace=True)
        _node_forward(ctx, mod, dims)
        ctx.want_feat = bool(features.requires_grad)
        return out

    @staticmethod
    def backward(ctx, g_tokens):
        B, V, h, w = ctx.dims
        g = g_tokens.to(dtype=torch.float32).contiguous()
        dfeat = torch.empty(B, V, ctx.mod.dim_out, h, w, device=g.device) if ctx.want_feat else None
        dw1, db1, dw2, db2 = _encoder_backward(ctx, g, dfeat)
        return None, dfeat, None, None, None, None, dw1, db1, dw2, db2


class _RayPeFpnFn(torch.autograd.Function):
    """tokens = the FPN neck's merged features + encoding as one autograd node (AddRayPE.tokens_from_pyramid): backward =
    parq_ray_pe_backward (encoder gradients) + parq_fpn_backward (the four level gradients, the adjoint of the resize)."""

    @staticmethod
    def forward(ctx, mod, layer, camera, T_cp, T_wp, T_wl, w1, b1, w2, b2, l0, l1, l2, l3):
        levels = (l0, l1, l2, l3)
        out, dims, _ = mod._run(camera, T_cp, T_wp, T_wl, tuple(levels[layer].shape[-2:]), None, own_workspace=True,
                                pyramid=(levels, layer))
        _node_forward(ctx, mod, dims)
        ctx.layer = layer
        ctx.level_shapes = tuple(tuple(lv.shape) for lv in levels)
        ctx.want_levels = tuple(bool(lv.requires_grad) for lv in levels)
        return out

    @staticmethod
    def backward(ctx, g_tokens):
        B, V = ctx.dims[:2]
        g = g_tokens.to(dtype=torch.float32).contiguous()
        dw1, db1, dw2, db2 = _encoder_backward(ctx, g, None)
        dlev = [None] * 4
        if any(ctx.want_levels):
            lib = _lib.load()
            d = [torch.empty(shape, dtype=torch.float32, device=g.device) for shape in ctx.level_shapes]
            _lib.check(lib.parq_fpn_backward(_lib.ptr(g), B, V, ctx.mod.dim_out, C.byref(_fpn_levels(d, ctx.layer)),
                                             (C.c_void_p * 4)(*(t.data_ptr() for t in d)), _lib.stream_ptr()), "parq_fpn_backward")
            dlev = [t if want else None for t, want in zip(d, ctx.want_levels)]
        return (None, None, None, None, None, None, dw1, db1, dw2, db2, *dlev)


def _fpn_levels(levels, layer):
    """parq_fpn_levels of four contiguous float32 CUDA tensors (B, T, C/4, h_l, w_l)."""
    st = _lib.ParqFpnLevels()
    for i, lv in enumerate(levels):
        st.level[i] = _lib.ptr(lv).value
        st.h[i], st.w[i] = int(lv.shape[-2]), int(lv.shape[-1])
    st.layer = int(layer)
    return st


class _WsHold:
    """The workspace one autograd node of AddRayPE reads in its backward, and the generation it was written in."""
    __slots__ = ("ws", "gen", "consumed", "__weakref__")

    def __init__(self, ws, gen):
        self.ws, self.gen, self.consumed = ws, gen, False


class AddRayPE(nn.Module):
    def __init__(self, dim_out: int, ray_points_scale=(-2, 2, -1.5, 0, 0.25, 4.25), num_samples: int = 64,
                 min_depth: float = 0.25, max_depth: float = 5.25):
        super().__init__()
        self.dim_out = dim_out
        self.ray_points_scale = [float(x) for x in ray_points_scale]
        self.num_samples = num_samples
        self.min_depth = float(min_depth)
        self.max_depth = float(max_depth)
        self.encoder = nn.Sequential(nn.Linear(3 * num_samples, dim_out), nn.ReLU(), nn.Linear(dim_out, dim_out))
        self._ws = None
        self._ws_key = None               # what the weight copies inside ``_ws`` were made from (see _run)
        self._ws_stream = None            # the launch stream ``_ws`` belongs to, and the parked (workspace, key) pairs of other streams:
        self._ws_parked = {}              # calls on different HIP streams (parq_amd.InFlight) each own their pose tables and weight copies
        self._gen = 0                     # forward counter, stamped on the workspace it wrote (``_parq_gen``)
        self._ws_owner = None             # weak reference to the _WsHold of the autograd node that owns ``_ws`` (if any)
        self.dp_all_reduce = False        # True: the backward all-reduces (mean) the encoder gradients over the default process group

    def _run(self, camera, T_cp, T_wp, T_wl, feat_hw, features, nchw=False, own_workspace=False, out_dtype=torch.float32,
             pyramid=None):
        cam, T_cp, T_wp, T_wl = (raw(x) for x in (camera, T_cp, T_wp, T_wl))
        if not cam.is_cuda:
            raise RuntimeError("parq_amd.AddRayPE runs on the GPU only (there is no CPU fallback)")
        dev = cam.device
        prep = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
        cam, T_cp, T_wp, T_wl = prep(cam), prep(T_cp), prep(T_wp), prep(T_wl)
        self._last_geo = (cam, T_cp, T_wp, T_wl)
        B, V = cam.shape[:2]
        if feat_hw is None:
            wf, hf = cam[0, 0, :2].tolist()                 # the reference rounds the first camera's size too (:80-81)
            feat_hw = (int(round(hf)), int(round(wf)))
        h, w = feat_hw
        Cd = self.dim_out
        if features is not None:
            features = prep(features)
            assert features.shape == (B, V, Cd, h, w), tuple(features.shape)
        if pyramid is not None:                              # (levels, layer): parq_ray_pe_fpn reads the four levels instead
            levels, layer = pyramid
            levels = [prep(lv) for lv in levels]
            assert not nchw and features is None and tuple(levels[layer].shape[-2:]) == (h, w)
            fpn = _fpn_levels(levels, layer)
        lib = _lib.load()
        self._gen += 1
        sid = int(torch.cuda.current_stream(dev).cuda_stream)
        if sid != self._ws_stream:        # another stream's call may still be reading this workspace: park it, take this stream's own
            if self._ws is not None:
                self._ws_parked[self._ws_stream] = (self._ws, self._ws_key)
            self._ws, self._ws_key = self._ws_parked.pop(sid, (None, None))
            self._ws_stream = sid
        # include/parq_hip.h: 1 = NCHW output, 2 = inference (the hidden layer is not kept for a backward: on the one-pass path it
        # never leaves the CU and the workspace shrinks by B*V*h*w*C floats)
        fused = Cd == 256 and self.num_samples == 64          # the library's one-pass path can write (B, V, C, h, w) directly
        nchw = bool(nchw and fused)
        flags = (1 if nchw else 0) | (0 if own_workspace else 2)
        # 8 / 16: fp16 / bf16 token rows, rounded to nearest in the kernel (inference, channels-last)
        out16 = {torch.float32: 0, torch.float16: 8, torch.bfloat16: 16}[out_dtype]
        assert not (out16 and (nchw or own_workspace)), "16-bit tokens: channels-last inference output only"
        flags |= out16
        nbytes = lib.parq_ray_pe_workspace_bytes_flags(B, V, h, w, Cd, self.num_samples, flags)
        owner = self._ws_owner() if self._ws_owner is not None else None
        if owner is not None and not owner.consumed and owner.ws is self._ws:
            self._ws = None                                  # an autograd node still needs the hidden layer saved there
        if self._ws is None or self._ws.numel() * 4 < nbytes or self._ws.device != dev:
            self._ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=dev)
            self._ws_key = None
        # the split / fragment-ordered weight copies inside the workspace are reused while the same workspace holds the same
        # weights (data pointer and version of the four parameters: optimizer steps and load_state_dict bump the version;
        # writes through .data need invalidate_weights()) in the same layout
        key = (self._ws.data_ptr(), flags & 2, B, V, h, w) + tuple((t.data_ptr(), t._version) for t in
                                                                     (self.encoder[0].weight, self.encoder[2].weight))
        if key == self._ws_key:
            flags |= 4
        self._ws_key = key
        out = torch.empty((B, V, Cd, h, w) if nchw else (B, V * h * w, Cd), dtype=out_dtype, device=dev)
        p = [prep(t.detach()) for t in (self.encoder[0].weight, self.encoder[0].bias, self.encoder[2].weight,
                                        self.encoder[2].bias)]
        if pyramid is not None:
            _lib.check(lib.parq_ray_pe_fpn(_lib.ptr(cam), _lib.ptr(T_cp), _lib.ptr(T_wp), _lib.ptr(T_wl), _lib.ptr(p[0]),
                                           _lib.ptr(p[1]), _lib.ptr(p[2]), _lib.ptr(p[3]), (C.c_float * 6)(*self.ray_points_scale),
                                           self.min_depth, self.max_depth, self.num_samples, B, V, h, w, Cd, C.byref(fpn),
                                           _lib.token_ptr(out), flags, _lib.ptr(self._ws), self._ws.numel() * 4, _lib.stream_ptr()),
                       "parq_ray_pe_fpn")
        else:
            _lib.check(lib.parq_ray_pe(_lib.ptr(cam), _lib.ptr(T_cp), _lib.ptr(T_wp), _lib.ptr(T_wl), _lib.ptr(p[0]),
                                       _lib.ptr(p[1]), _lib.ptr(p[2]), _lib.ptr(p[3]), (C.c_float * 6)(*self.ray_points_scale),
                                       self.min_depth, self.max_depth, self.num_samples, B, V, h, w, Cd, _lib.ptr(features),
                                       _lib.token_ptr(out), flags, _lib.ptr(self._ws), self._ws.numel() * 4, _lib.stream_ptr()),
                       "parq_ray_pe")
        self._ws._parq_gen = self._gen
        return out, (B, V, h, w), nchw

    def invalidate_weights(self):
        """After parameter writes that bypass autograd's version counter (``p.data.copy_()``, EMA swaps through ``.data``)."""
        self._ws_key = None

    def _needs_graph(self, features=None):
        return torch.is_grad_enabled() and (self.training or any(p.requires_grad for p in self.parameters())
                                            or bool(getattr(features, "requires_grad", False)))

    def forward(self, images_feat, camera=None, T_camera_pseudoCam=None, T_world_pseudoCam=None, T_world_local=None):
        """The encoding (B, T, C, H, W), as the reference returns it (images_feat only supplies the shape).  With gradients
        enabled and an encoder parameter that requires grad the result carries a graph, as the reference's does
        (model/ray_positional_encoding.py:128-136): the same autograd node as ``tokens`` on zero feature maps."""
        hw = tuple(images_feat.shape[-2:])
        if self._needs_graph():
            B, V = raw(camera).shape[:2]
            zeros = torch.zeros(B, V, self.dim_out, hw[0], hw[1], dtype=torch.float32, device=raw(camera).device)
            tok = self.tokens(zeros, camera, T_camera_pseudoCam, T_world_pseudoCam, T_world_local)
            return tok.view(B, V, hw[0], hw[1], self.dim_out).permute(0, 1, 4, 2, 3)
        with torch.no_grad():
            enc, (B, V, h, w), nchw = self._run(camera, T_camera_pseudoCam, T_world_pseudoCam, T_world_local, hw, None, nchw=True)
            return enc if nchw else enc.view(B, V, h, w, self.dim_out).permute(0, 1, 4, 2, 3)

    def tokens(self, images_feat, camera, T_camera_pseudoCam, T_world_pseudoCam, T_world_local, dtype=None):
        """features + encoding, tokenised channels-last (B, T*H*W, C) in one pass.  With gradients enabled and anything to
        differentiate (train mode, an encoder parameter or the feature maps requiring grad — eval mode included, like the
        reference) the call is an autograd node that owns the workspace holding the hidden layer for its backward.
        ``dtype`` (None = float32): torch.float16 / torch.bfloat16 tokens — written as such by the kernel on the inference path
        (each element the float32 result rounded to nearest, i.e. equal to ``tokens(...).to(dtype)``), the float32 autograd node
        followed by ``.to(dtype)`` with a graph."""
        if dtype is not None and dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError("AddRayPE.tokens: dtype must be None, torch.float32, torch.float16 or torch.bfloat16")
        if self._needs_graph(images_feat):
            e0, e2 = self.encoder[0], self.encoder[2]
            out = _RayPeFn.apply(self, images_feat, camera, T_camera_pseudoCam, T_world_pseudoCam, T_world_local,
                                 e0.weight, e0.bias, e2.weight, e2.bias)
            return out if dtype in (None, torch.float32) else out.to(dtype)
        with torch.no_grad():
            hw = tuple(images_feat.shape[-2:])
            out, _, _ = self._run(camera, T_camera_pseudoCam, T_world_pseudoCam, T_world_local, hw, images_feat,
                                  out_dtype=dtype or torch.float32)
            return out

    def tokens_from_pyramid(self, levels, layer, camera, T_camera_pseudoCam, T_world_pseudoCam, T_world_local, dtype=None):
        """``tokens`` of the FPN neck's output without building it: ``levels`` are the four FPN levels '0'..'3' as
        (B, T, C/4, h_l, w_l) tensors; the result equals ``tokens(torch.cat([F.interpolate(lv.flatten(0, 1), levels[layer].shape[-2:],
        mode="bilinear").unflatten(0, (B, T)) for lv in levels], 2), ...)`` (model/resnet_fpn.py:62-91 of the reference), with the
        resize computed where the kernel reads the features — the resized stack is never written.  With anything to differentiate
        it is one autograd node (encoder and level gradients; the level gradients have no atomics and are bit-identical run to
        run).  fp16 / bf16 levels are upcast to float32 with a copy first (the kernels read float32 levels)."""
        if dtype is not None and dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError("AddRayPE.tokens_from_pyramid: dtype must be None, torch.float32, torch.float16 or torch.bfloat16")
        levels = self._check_pyramid(levels, layer, camera)
        levels = [lv if lv.dtype == torch.float32 else lv.to(torch.float32) for lv in levels]
        if self._needs_graph() or (torch.is_grad_enabled() and any(lv.requires_grad for lv in levels)):
            e0, e2 = self.encoder[0], self.encoder[2]
            out = _RayPeFpnFn.apply(self, layer, camera, T_camera_pseudoCam, T_world_pseudoCam, T_world_local,
                                    e0.weight, e0.bias, e2.weight, e2.bias, *levels)
            return out if dtype in (None, torch.float32) else out.to(dtype)
        with torch.no_grad():
            out, _, _ = self._run(camera, T_camera_pseudoCam, T_world_pseudoCam, T_world_local, tuple(levels[layer].shape[-2:]),
                                  None, out_dtype=dtype or torch.float32, pyramid=(levels, layer))
            return out

    def _check_pyramid(self, levels, layer, camera):
        """Argument checks of tokens_from_pyramid (ValueError), before anything needs the GPU."""
        if isinstance(layer, bool) or not isinstance(layer, int) or not 0 <= layer <= 3:
            raise ValueError("AddRayPE.tokens_from_pyramid: layer must be an int in 0..3, got %r" % (layer,))
        if isinstance(levels, (str, bytes)) or not hasattr(levels, "__len__") or len(levels) != 4:
            raise ValueError("AddRayPE.tokens_from_pyramid: levels must be a sequence of exactly four tensors (FPN levels '0'..'3')")
        levels = list(levels)
        for i, lv in enumerate(levels):
            if not isinstance(lv, torch.Tensor) or lv.dim() != 5:
                raise ValueError("AddRayPE.tokens_from_pyramid: level %d must be a (B, T, C/4, h, w) tensor" % i)
            if lv.dtype not in (torch.float32, torch.float16, torch.bfloat16):
                raise ValueError("AddRayPE.tokens_from_pyramid: level %d has dtype %s (float32, float16 or bfloat16)" % (i, lv.dtype))
            if min(lv.shape) < 1:
                raise ValueError("AddRayPE.tokens_from_pyramid: level %d is empty: %s" % (i, tuple(lv.shape)))
        B, T, cl = levels[0].shape[:3]
        if any(tuple(lv.shape[:3]) != (B, T, cl) for lv in levels):
            raise ValueError("AddRayPE.tokens_from_pyramid: the levels disagree in (B, T, C/4): %s" % [tuple(lv.shape[:3]) for lv in levels])
        if 4 * cl != self.dim_out or cl % 16 != 0:
            raise ValueError("AddRayPE.tokens_from_pyramid: four levels of %d channels for C = %d (C/4 must be a multiple of 16)"
                             % (cl, self.dim_out))
        cam = raw(camera)
        if tuple(cam.shape[:2]) != (B, T):
            raise ValueError("AddRayPE.tokens_from_pyramid: levels are (B, T) = %s but the camera is %s" % ((B, T), tuple(cam.shape[:2])))
        if any(lv.device != cam.device for lv in levels):
            raise ValueError("AddRayPE.tokens_from_pyramid: the levels and the camera are on different devices")
        return levels
