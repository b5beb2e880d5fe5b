"""ViewWindow: a streaming window of V view slots over one PARQDecoder (video inference).

A video server keeps a window of V key frames and replaces one or a few of them per step.  ``PARQDecoder.forward`` pays for all V
views every call: the hoisted K/V projection runs over all ``V*h*w`` tokens.  A window owns the token buffer, the camera / pose
tables and ONE inference workspace (outside the decoder's ``max_workspaces`` cache), remembers which slots were replaced since its
last forward and re-projects only those (include/parq_hip.h parq_forward_views); the iterations run as always.  The outputs are the
bits of ``decoder.forward`` on the assembled inputs.

One rule the caller must know: the tokens of a view are NOT independent of the snippet.  The ray points of the positional encoding
are expressed in the local frame (``T_local_world @ T_world_pseudoCam``), so a view's tokens change with ``T_world_local``.  A window
therefore lives in one fixed local frame; ``rebase`` starts a new one and every slot has to be put again.  At this level tokens are
opaque: that they were encoded with the window's ``T_world_local`` is the caller's responsibility (``PARQ.view_window`` encodes them
itself and guarantees it).

This module imports without a GPU; ``slot_runs`` / ``row_ranges`` and the argument checks are pure.
"""
from __future__ import annotations

import weakref

import torch

from .wrappers import raw

TOKEN_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def slot_runs(slots):
    """Maximal runs of adjacent slots: [(first, last)] inclusive, ascending."""
    out = []
    for s in sorted(set(int(x) for x in slots)):
        if out and s == out[-1][1] + 1:
            out[-1] = (out[-1][0], s)
        else:
            out.append((s, s))
    return out


def row_ranges(slots, V, hw, tile):
    """The token-row ranges [r0, r1) per scene that a forward re-projects for the dirty `slots` of a window of V views with `hw`
    keys each: adjacent slots merge into runs, every run is widened outward to a multiple of `tile` rows (the granularity of the
    projection kernel: 64 for model dims 128 / 256, 128 for the tiled kernel, 32 above dim 256) and clamped to N = V*hw; ranges that
    touch after widening merge.  The library computes the same (api.hip view_row_runs) and reports the row total."""
    N = int(V) * int(hw)
    out = []
    for a, b in slot_runs(slots):
        if a < 0 or b >= V:
            raise ValueError("slot outside [0, %d)" % V)
        r0 = (a * hw) // tile * tile
        r1 = min(N, -(-((b + 1) * hw) // tile) * tile)
        if out and r0 <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], r1))
        else:
            out.append((r0, r1))
    return out


def check_window_args(B, V, h, w, C_, T_world_local, dtype):
    """Argument checks of a window's construction (ValueError), before anything needs the GPU.  Returns T_world_local as (B, 1, 12)."""
    for name, v in (("B", B), ("V", V)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError("ViewWindow: %s must be a positive int, got %r" % (name, v))
    for name, v in (("h", h), ("w", w)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 2:
            raise ValueError("ViewWindow: %s must be an int >= 2, got %r" % (name, v))
    if dtype not in TOKEN_DTYPES:
        raise ValueError("ViewWindow: dtype must be torch.float32, torch.float16 or torch.bfloat16, got %r" % (dtype,))
    if (V * h * w * C_) % 8 != 0:
        raise ValueError("ViewWindow: V*h*w*C must be a multiple of 8")
    T = raw(T_world_local)
    if not isinstance(T, torch.Tensor) or T.shape not in ((B, 12), (B, 1, 12)):
        raise ValueError("ViewWindow: T_world_local must be (B, 12) or (B, 1, 12) = (%d, [1,] 12), got %s"
                         % (B, tuple(getattr(T, "shape", ()))))
    if not T.is_cuda:
        raise ValueError("ViewWindow: T_world_local is on %s; a window lives on the GPU (there is no CPU fallback)" % T.device)
    return T.reshape(B, 1, 12)


def check_put_args(B, V, h, w, C_, dtype, device, slot, tokens, camera, T_camera_pseudoCam, T_world_pseudoCam, what="tokens"):
    """Argument checks of ``put`` / ``put_features`` (ValueError), before anything needs the GPU: slots, then dtype, shapes and
    devices.  `tokens` None: only the slots and the three tables are checked.  Returns (slots, camera, T_cp, T_wp) as raw tensors."""
    slots = [slot] if isinstance(slot, int) and not isinstance(slot, bool) else list(slot) if isinstance(slot, (list, tuple, range)) else None
    if slots is None or not slots or any(isinstance(s, bool) or not isinstance(s, int) for s in slots):
        raise ValueError("ViewWindow.put: slot must be an int or a non-empty list of ints, got %r" % (slot,))
    if any(s < 0 or s >= V for s in slots):
        raise ValueError("ViewWindow.put: slot %r outside [0, %d)" % (slots, V))
    if len(set(slots)) != len(slots):
        raise ValueError("ViewWindow.put: slot %r lists a slot twice" % (slots,))
    n, hw = len(slots), h * w
    cam, T_cp, T_wp = raw(camera), raw(T_camera_pseudoCam), raw(T_world_pseudoCam)
    if tokens is not None:
        if not isinstance(tokens, torch.Tensor) or tokens.dtype != dtype:
            raise ValueError("ViewWindow.put: %s must be a %s tensor (the window's dtype), got %s"
                             % (what, dtype, getattr(tokens, "dtype", type(tokens))))
        if tuple(tokens.shape) not in ((B, n * hw, C_), (B, n, hw, C_)):
            raise ValueError("ViewWindow.put: %s must be (B, len(slots)*h*w, C) = %s or (B, len(slots), h*w, C), got %s"
                             % (what, (B, n * hw, C_), tuple(tokens.shape)))
    for name, t, width in (("camera", cam, 6), ("T_camera_pseudoCam", T_cp, 12), ("T_world_pseudoCam", T_wp, 12)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, n, width):
            raise ValueError("ViewWindow.put: %s must be (B, len(slots), %d) = %s, got %s"
                             % (name, width, (B, n, width), tuple(getattr(t, "shape", ()))))
        if not t.dtype.is_floating_point:
            raise ValueError("ViewWindow.put: %s must be a floating-point tensor, got %s" % (name, t.dtype))
    for name, t in ((what, tokens), ("camera", cam), ("T_camera_pseudoCam", T_cp), ("T_world_pseudoCam", T_wp)):
        if t is not None and t.device != device:
            raise ValueError("ViewWindow.put: %s is on %s, the window on %s (a CPU tensor is not moved for you)" % (name, t.device, device))
    return slots, cam, T_cp, T_wp


class ViewWindow:
    """``decoder.view_window(B, V, h, w, T_world_local, dtype=torch.float32)``.

    ``put(slot, tokens, camera, T_camera_pseudoCam, T_world_pseudoCam)`` copies one or several views into their slots and marks them
    dirty; ``forward()`` returns the list of per-iteration dicts of ``decoder.forward`` on the window's present contents, projecting
    K / V of the dirty slots only (``last_projected_views``, ``last_projected_rows``: token rows per scene after widening to the
    projection kernel's granularity; N in attention mode "fp32", which keeps no cache to patch).  ALL slots are projected before the
    first forward, after ``rebase`` and whenever the decoder is not in the state the cache was built in — weights version,
    ``attention_mode``, ``safe_heads``, ``fuse_seams``, ``batch_invariant``, token type, ``range_check`` switched to or from "off" —
    and after a forward that raised a range / too-peaked flag.  ``range_check`` holds as for ``forward``: under "sync" a window
    forward never returns NaN (a flagged forward is re-run with everything its fallback changed); under "lazy" / "off" a raised flag
    leaves all slots dirty — as soon as the host can see it: a forward enqueued while the flagged one is still in flight lists its
    dirty slots only, and is NaN all the same, because a forward that skips rows keeps the device's range flag (include/parq_hip.h).
    From the second forward of a kind on the iterations replay from the captured graph.
    ``decoder.cross_attention_map()`` / ``cross_attention_view_mass()`` describe the window's forward when it was the decoder's last
    one on the stream; their view index is the slot index.  A window is bound to the stream that was current when it was made: calls
    from another stream are ordered behind it and it behind them.  Not for use under ``InFlight``."""

    def __init__(self, decoder, B, V, h, w, T_world_local, dtype=torch.float32):
        C_ = decoder.dim_in
        T = check_window_args(B, V, h, w, C_, T_world_local, dtype)
        dev = T.device
        self._dec = decoder
        self.B, self.V, self.h, self.w, self.dtype = B, V, h, w, dtype
        self._dev = dev
        self._stream = torch.cuda.current_stream(dev)
        self._raw = int(self._stream.cuda_stream)
        with torch.cuda.device(dev):
            self._tokens = torch.zeros(B, V * h * w, C_, dtype=dtype, device=dev)
            self._camera = torch.zeros(B, V, 6, dtype=torch.float32, device=dev)
            self._T_cp = torch.zeros(B, V, 12, dtype=torch.float32, device=dev)
            self._T_wp = torch.zeros(B, V, 12, dtype=torch.float32, device=dev)
            self._T_wl = T.to(torch.float32).contiguous().clone()
        self._slot = decoder._free_slot()
        decoder.__dict__.setdefault("_windows", weakref.WeakSet()).add(self)
        self._entry = None                 # decoder._WsEntry of the window's workspace (allocated by the first forward)
        self._built = None                 # the decoder state the cache in it was built in
        self._dirty = set(range(V))
        self._unput = set(range(V))        # slots not put since the window was made / rebased
        self._sc = None
        self._closed = False
        self.last_projected_views = None
        self.last_projected_rows = None

    # ------------------------------------------------------------------ what the window holds: aliases of its buffers, for READING only —
    # do not write through them (a write changes what the next forward reads without marking the slot dirty: use put); copying
    # the token buffer for every look would cost more than the window saves
    tokens = property(lambda self: self._tokens.detach())
    camera = property(lambda self: self._camera.detach())
    T_camera_pseudoCam = property(lambda self: self._T_cp.detach())
    T_world_pseudoCam = property(lambda self: self._T_wp.detach())
    T_world_local = property(lambda self: self._T_wl.detach())

    @property
    def dirty_slots(self):
        """The slots the next ``forward`` projects as far as the window knows now (all of them when the last forward raised a flag;
        a pending change of the decoder's state is only seen by ``forward`` itself)."""
        return list(range(self.V)) if self._flag_raised() else sorted(self._dirty)

    def invalidate(self):
        """Project every slot again at the next ``forward`` (the tokens stay): for a cache that may no longer match the tokens or
        the weights for a reason the window cannot see, e.g. parameter writes through ``.data`` (``decoder.invalidate_weights()``)."""
        self._dirty = set(range(self.V))

    def _flag_raised(self):
        m = self._dec._mirror_np
        return self._entry is not None and m is not None and int(m[self._slot]) != 0

    def _alive(self):
        if self._closed:
            raise RuntimeError("ViewWindow: the window was closed")

    class _OnStream:
        """Run a block on the window's stream, ordered behind the caller's current stream, and the caller's behind it."""

        def __init__(self, win):
            self.win = win

        def __enter__(self):
            w = self.win
            # (the usual case — the caller is on the window's stream — costs one raw-stream query: under range_check = "sync" the
            # device idles while the host prepares a forward, so host time in front of the first launch is wall time)
            self.other = torch._C._cuda_getCurrentRawStream(w._dev.index) != w._raw
            if self.other:
                self.cur = torch.cuda.current_stream(w._dev)
                w._stream.wait_stream(self.cur)
                self.ctx = torch.cuda.stream(w._stream)
                self.ctx.__enter__()
            return self

        def __exit__(self, *exc):
            if self.other:
                self.ctx.__exit__(*exc)
                self.cur.wait_stream(self.win._stream)
            return False

    # ------------------------------------------------------------------ filling
    def _store(self, slots, tok4, cam, T_cp, T_wp):
        B, V, hw = self.B, self.V, self.h * self.w
        buf = self._tokens.view(B, V, hw, -1)
        if slots == list(range(slots[0], slots[0] + len(slots))):          # one ascending run (a single slot, a refill): four copies
            sl = slice(slots[0], slots[0] + len(slots))
            buf[:, sl].copy_(tok4)
            self._camera[:, sl].copy_(cam)
            self._T_cp[:, sl].copy_(T_cp)
            self._T_wp[:, sl].copy_(T_wp)
        else:
            for i, s in enumerate(slots):
                buf[:, s].copy_(tok4[:, i])
                self._camera[:, s].copy_(cam[:, i])
                self._T_cp[:, s].copy_(T_cp[:, i])
                self._T_wp[:, s].copy_(T_wp[:, i])
        self._dirty.update(slots)
        self._unput.difference_update(slots)

    @torch.no_grad()
    def put(self, slot, tokens, camera, T_camera_pseudoCam, T_world_pseudoCam):
        """Replace the views in `slot` (an int or a list of ints): `tokens` (B, len(slots)*h*w, C) or (B, len(slots), h*w, C) in the
        window's dtype — encoded with the window's ``T_world_local`` — and the (B, len(slots), .) camera and pose rows."""
        self._alive()
        slots, cam, T_cp, T_wp = check_put_args(self.B, self.V, self.h, self.w, self._dec.dim_in, self.dtype, self._dev, slot,
                                                tokens, camera, T_camera_pseudoCam, T_world_pseudoCam)
        with self._OnStream(self):
            self._store(slots, tokens.reshape(self.B, len(slots), self.h * self.w, -1), cam, T_cp, T_wp)

    @torch.no_grad()
    def rebase(self, T_world_local):
        """A new local frame: every slot becomes dirty and has to be put again (its tokens were encoded in the old frame); a
        ``forward`` before that raises."""
        self._alive()
        T = check_window_args(self.B, self.V, self.h, self.w, self._dec.dim_in, T_world_local, self.dtype)
        if T.device != self._dev:
            raise ValueError("ViewWindow.rebase: T_world_local is on %s, the window on %s" % (T.device, self._dev))
        with self._OnStream(self):
            self._T_wl.copy_(T)
        self._dirty = set(range(self.V))
        self._unput = set(range(self.V))

    # ------------------------------------------------------------------ forward
    def _state_key(self, tt):
        d = self._dec
        return (d._arena_gen, d._mode_set, d._tiers_set, d._seams_set, d._inv_set, tt)

    def _enqueue(self, flat):
        from . import _lib
        from .decoder import TOKEN_TYPES, _WsEntry, _raw_stream
        dec, dev = self._dec, self._dev
        lib = _lib.load()
        hd = dec._handle()                                   # applies pending settings (mode, tiers, seams, batch invariance)
        tt = TOKEN_TYPES[self.dtype]
        dec._token_type(hd, tt)                              # (before the workspace is sized: mode "fp32" carves a widened copy)
        nbytes = lib.parq_workspace_bytes(hd, self.B, self.V, self.h, self.w)
        if nbytes == 0:
            raise RuntimeError("parq_workspace_bytes returned 0 for B=%d V=%d h=%d w=%d" % (self.B, self.V, self.h, self.w))
        if self._entry is None or self._entry.ws.numel() * 4 != nbytes:
            if self._entry is not None and self._entry.graphs:
                dec._retire_graphs(self._entry)              # the workspace is carved differently in this state: a new one
            self._entry = _WsEntry(torch.empty(nbytes // 4, dtype=torch.float32, device=dev), self._slot, self._stream)
            self._built = None
        if self._sc is None:
            self._sc = _lib.ParqScene(self.B, self.V, self.h, self.w, _lib.token_ptr(self._tokens), _lib.ptr(self._camera),
                                      _lib.ptr(self._T_cp), _lib.ptr(self._T_wp), _lib.ptr(self._T_wl))
        key = self._state_key(tt)                            # the keys the library's validity record holds (and seam fusion)
        if key != self._built:
            self._dirty = set(range(self.V))
        views = sorted(self._dirty)
        keep = (self._tokens, self._camera, self._T_cp, self._T_wp, self._T_wl)
        run = dec._enqueue_forward(self._sc, keep, flat, dev, entry=self._entry, views=views)
        dec.__dict__["_map_window"] = ((self.B, self.V, self.h, self.w, dev.index, _raw_stream(dev)), self._entry)
        self._built = self._state_key(tt)
        self._dirty = set()
        self.last_projected_views, self.last_projected_rows = run.views, run.rows      # (all views if the library refused the subset)
        return run

    @torch.no_grad()
    def forward(self):
        """The decoder's forward on the window's contents: a list of per-iteration dicts, as ``PARQDecoder.forward`` returns."""
        from .decoder import OUTPUT_KEYS
        self._alive()
        dec, dev = self._dec, self._dev
        if dec._defer is not None:
            raise RuntimeError("ViewWindow.forward under InFlight is out of scope: a window is bound to its own stream")
        if self._unput:
            raise RuntimeError("ViewWindow.forward: slots %s have not been put since the window was %s (their tokens belong to "
                               "another local frame)" % (sorted(self._unput), "made" if self._built is None else "made or rebased"))
        with self._OnStream(self) as on:
            dec._check_mode()
            if self._flag_raised():
                self._dirty = set(range(self.V))             # the flagged forward's range flag must be raised again, not skipped
            dec._range_poll()
            dec._ensure_packed(dev)
            dec._order_behind_pack(dev)
            L, B, Q = dec.num_layers, self.B, dec.num_queries
            flat = torch.empty(L * B * Q * dec._out_width, dtype=torch.float32, device=dev)
            run = self._enqueue(flat)
            for _attempt in range(dec.num_heads + 2):        # "sync" (and every module's first forward): wait, look, re-run
                if not dec._range_after_forward(run, self._sc, dev):
                    break
                run = self._enqueue(flat)                    # the fallback changed the state: every slot is projected again
            if on.other:
                flat.record_stream(on.cur)
        ncls = dec.num_semcls + 1
        widths = (ncls, 3, 3, 6, ncls, 3)
        rows = L * B * Q
        per = [seg.view(L, B, Q, wd).unbind(0) for seg, wd in zip(flat.split([rows * wd for wd in widths]), widths)]
        return [dict(zip(OUTPUT_KEYS, [p[i] for p in per])) for i in range(L)]

    __call__ = forward

    def close(self):
        """Release the workspace (and its captured graphs, once the stream has passed them)."""
        if self._closed:
            return
        self._closed = True
        dec = self._dec
        if self._entry is not None and self._entry.graphs:
            dec._retire_graphs(self._entry)
        mw = dec.__dict__.get("_map_window")
        if mw is not None and mw[1] is self._entry:
            dec.__dict__["_map_window"] = None
        self._entry = None
        dec.__dict__.get("_windows", set()).discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:                                    # noqa: BLE001 - interpreter shutdown
            pass


class FeatureViewWindow(ViewWindow):
    """``PARQ.view_window(B, V, h, w, T_world_local)``: a ViewWindow that encodes the views itself — ``put_features`` runs the ray-PE
    tokenisation for the put views only, with the window's ``T_world_local`` (so the fixed-frame rule holds by construction), in the
    module's ``token_dtype``."""

    def __init__(self, module, B, V, h, w, T_world_local):
        super().__init__(module.box3d_decoder, B, V, h, w, T_world_local, module.token_dtype or torch.float32)
        self._pe = module.add_ray_pe
        self._module = module
        self.frame_prep = None             # the FramePrep of put_frames (made at its first call: parq_amd.FramePrep(); assign another)

    @torch.no_grad()
    def put_features(self, slot, features_or_pyramid, camera, T_camera_pseudoCam, T_world_pseudoCam):
        """`features_or_pyramid`: the put views' feature maps (B, len(slots), C, h, w), or ``(levels, layer)`` with the four FPN
        levels (B, len(slots), C/4, h_l, w_l) of those views (``AddRayPE.tokens_from_pyramid``).  One temporary of the put views'
        tokens and a strided copy into the slots."""
        self._alive()
        slots, cam, T_cp, T_wp = check_put_args(self.B, self.V, self.h, self.w, self._dec.dim_in, self.dtype, self._dev, slot,
                                                None, camera, T_camera_pseudoCam, T_world_pseudoCam)
        n = len(slots)
        pyramid = isinstance(features_or_pyramid, (tuple, list)) and len(features_or_pyramid) == 2 and isinstance(features_or_pyramid[1], int)
        if pyramid:
            levels, layer = features_or_pyramid
            if not 0 <= layer <= 3 or len(levels) != 4 or any(not isinstance(lv, torch.Tensor) or lv.dim() != 5 for lv in levels) or \
                    tuple(levels[layer].shape[-2:]) != (self.h, self.w) or any(tuple(lv.shape[:2]) != (self.B, n) for lv in levels):
                raise ValueError("ViewWindow.put_features: (levels, layer) must be four (B, len(slots), C/4, h_l, w_l) levels with "
                                 "level `layer` of size %s" % ((self.h, self.w),))
            for i, lv in enumerate(levels):
                if lv.device != self._dev:
                    raise ValueError("ViewWindow.put_features: level %d is on %s, the window on %s" % (i, lv.device, self._dev))
        else:
            f = features_or_pyramid
            if not isinstance(f, torch.Tensor) or tuple(f.shape) != (self.B, n, self._dec.dim_in, self.h, self.w):
                raise ValueError("ViewWindow.put_features: features must be (B, len(slots), C, h, w) = %s, got %s"
                                 % ((self.B, n, self._dec.dim_in, self.h, self.w), tuple(getattr(f, "shape", ()))))
            if f.device != self._dev:
                raise ValueError("ViewWindow.put_features: features are on %s, the window on %s" % (f.device, self._dev))
        with self._OnStream(self):
            if pyramid:
                tok = self._pe.tokens_from_pyramid(levels, layer, cam, T_cp, T_wp, self._T_wl, dtype=self.dtype)
            else:
                tok = self._pe.tokens(features_or_pyramid, cam, T_cp, T_wp, self._T_wl, dtype=self.dtype)
            self._store(slots, tok.view(self.B, n, self.h * self.w, -1), cam, T_cp, T_wp)

    @torch.no_grad()
    def put_frames(self, slot, frames, intrinsics, T_world_camera):
        """Replace the views in `slot` from raw frames: `frames` (B, len(slots), H, W, 3) uint8 on the window's device, `intrinsics`
        (B, len(slots), 3, 3) of the frames as they are and `T_world_camera` (B, len(slots), 4, 4).  ``self.frame_prep``
        (``parq_amd.FramePrep()`` unless another was assigned: size, border, up axis, whose intrinsics) prepares the put views only,
        the module's ``backbone2d`` runs on them and the result — ``all_features`` or ``(fpn_features, fpn_layer)``, with
        ``camera_feature`` and the two pose tables — goes to ``put_features``.  The window's ``T_world_local`` stays what it was
        given (the prepared views' own local frame is not used).  ValueError when the module has no ``backbone2d``."""
        self._alive()
        backbone = self._module.backbone2d
        if backbone is None:
            raise ValueError("ViewWindow.put_frames: the module has no backbone2d to turn images into features (use put_features)")
        n = 1 if isinstance(slot, int) and not isinstance(slot, bool) else len(slot) if isinstance(slot, (list, tuple, range)) else -1
        if not isinstance(frames, torch.Tensor) or frames.ndim != 5 or tuple(frames.shape[:2]) != (self.B, n):
            raise ValueError("ViewWindow.put_frames: frames must be (B, len(slots), H, W, 3) with (B, len(slots)) = %s, got %s"
                             % ((self.B, n), tuple(getattr(frames, "shape", ()))))
        if frames.device != self._dev:
            raise ValueError("ViewWindow.put_frames: the frames are on %s, the window on %s" % (frames.device, self._dev))
        if self.frame_prep is None:
            from .frames import FramePrep
            self.frame_prep = FramePrep()
        batch = self.frame_prep(frames, intrinsics, T_world_camera)
        del batch["T_world_local"]
        batch = backbone(batch)
        feats = (batch["fpn_features"], batch["fpn_layer"]) if "fpn_features" in batch else batch["all_features"]
        self.put_features(slot, feats, batch["camera_feature"], batch["T_camera_pseudoCam"], batch["T_world_pseudoCam"])
