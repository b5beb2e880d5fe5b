"""Detections followed across snippets on the device: a scene-level list of objects with stable ids.

The reference merges the boxes predicted on successive snippets of a scene into tracks on the host (utils/f1_eval.py:293-352
``matching_pred``: oriented-box IoU matrix, Hungarian assignment on -IoU, match at IoU >= 0.1, the more confident observation
represents the track, unmatched detections open new tracks), and only inside its evaluator.  ``SceneTracks`` keeps the tracks of
every scene in device memory and does the whole step in one enqueue per snippet batch (include/parq_hip.h parq_tracks_update,
csrc/tracks.hip: select + compact, IoU over pairs, assignment + update): no copy to the host, no synchronisation, and a track id
per query comes back as a device tensor.  The rule, stated in full, is in the header; its NumPy statement is
tests/scene_tracks_cases.py.  One difference from the reference: tracks born in the same step are numbered in query order (the
reference puts never-assigned detections before assigned-under-threshold ones), so their ids can be permuted among themselves; the
set of tracks, and every metric, is the same.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_SIDE = 2048           # queries per scene and tracks per scene the kernels take


def check_tracks_args(corners_world, sem_cls_prob, pred_mask, n_names, num_classes):
    """Shapes / dtypes of one update (ValueError before anything touches the GPU); returns (B, Q)."""
    if not (torch.is_tensor(corners_world) and corners_world.ndim == 4 and tuple(corners_world.shape[2:]) == (8, 3)):
        raise ValueError("corners_world must be a (B, Q, 8, 3) tensor, got %s" % (tuple(getattr(corners_world, "shape", ())),))
    B, Q = corners_world.shape[:2]
    if not corners_world.is_floating_point():
        raise ValueError("corners_world must be floating-point, got %s" % corners_world.dtype)
    if not (torch.is_tensor(sem_cls_prob) and tuple(sem_cls_prob.shape) == (B, Q, num_classes) and sem_cls_prob.is_floating_point()):
        raise ValueError("sem_cls_prob must be a floating-point (B, Q, %d) tensor for B = %d, Q = %d, got %s"
                         % (num_classes, B, Q, tuple(getattr(sem_cls_prob, "shape", ()))))
    if not (torch.is_tensor(pred_mask) and tuple(pred_mask.shape) == (B, Q) and pred_mask.dtype in (torch.bool, torch.uint8)):
        raise ValueError("pred_mask must be a bool or uint8 (B, Q) tensor for B = %d, Q = %d" % (B, Q))
    if n_names != B:
        raise ValueError("%d scene names for a batch of %d scenes" % (n_names, B))
    if not 1 <= Q <= MAX_SIDE:
        raise ValueError("Q = %d: the tracker takes 1 to %d queries per scene" % (Q, MAX_SIDE))
    return B, Q


class SceneTracks:
    """A device-resident track store: ``update`` follows the detections of a snippet batch, ``boxes`` / ``to_host`` read the scenes'
    objects.  ``max_tracks`` is the capacity per scene (at most 2048): a detection that would open a track beyond it gets id -2 and
    is counted in ``dropped()`` — the store never overflows silently.  ``num_classes`` counts the background class, which is the
    last one.  Nothing here synchronises except ``to_host`` and ``dropped``."""

    def __init__(self, max_tracks=512, conf_thresh=0.1, iou_thresh=0.1, num_classes=10, device="cuda"):
        if isinstance(max_tracks, bool) or not isinstance(max_tracks, int) or not 1 <= max_tracks <= MAX_SIDE:
            raise ValueError("max_tracks must be an integer in [1, %d], got %r" % (MAX_SIDE, max_tracks))
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 2:
            raise ValueError("num_classes must be an integer >= 2 (the last class is the background), got %r" % (num_classes,))
        self.max_tracks = max_tracks
        self.conf_thresh = float(conf_thresh)
        self.iou_thresh = float(iou_thresh)
        self.num_classes = num_classes
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("parq_amd.SceneTracks lives on a GPU (device=%r): there is no CPU fallback" % (device,))
        self._words = 2 + 26 * max_tracks
        self._slots = {}                       # scene name -> slot
        self._store = None                     # (S_cap, words) int32
        self._ws = None
        self.enqueues = 0                      # parq_tracks_update calls so far

    # ---- the store -----------------------------------------------------------------------------------------------------
    def _grow(self, need):
        cap = 0 if self._store is None else self._store.shape[0]
        if need <= cap:
            return
        new_cap = max(need, 2 * cap, 8)
        lib = _lib.load()
        assert lib.parq_tracks_store_bytes(new_cap, self.max_tracks) == new_cap * self._words * 4
        store = torch.zeros(new_cap, self._words, dtype=torch.int32, device=self.device)
        if cap:
            store[:cap].copy_(self._store)      # device to device, ordered on the stream: no synchronisation
        self._store = store

    def _slot(self, name):
        if name not in self._slots:
            self._slots[name] = len(self._slots)
        return self._slots[name]

    def _views(self, slot):
        mt = self.max_tracks
        row = self._store[slot]
        return {"count": row[0], "dropped": row[1], "labels": row[2:2 + mt], "scores": row[2 + mt:2 + 2 * mt].view(torch.float32),
                "corners": row[2 + 2 * mt:].view(torch.float32).view(mt, 8, 3)}

    # ---- one snippet batch -----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, scene_names, corners_world, sem_cls_prob, pred_mask, iou_out=None):
        """scene_names [B]; corners_world (B,Q,8,3); sem_cls_prob (B,Q,num_classes); pred_mask (B,Q) bool / uint8 -> track_id (B,Q)
        int32 on the device: the track of each detection, -1 for a query that is no detection, -2 for a detection the full store
        could not take.  A name listed k times is processed in k enqueues, each seeing what the previous one left.  ``iou_out``
        (tests): a float32 (B, Q, max_tracks) device tensor that receives the IoU matrices."""
        names = list(scene_names)
        B, Q = check_tracks_args(corners_world, sem_cls_prob, pred_mask, len(names), self.num_classes)
        if self.device.index is None and corners_world.is_cuda:
            self.device = corners_world.device                    # "cuda": the device of the first batch
        for t in (corners_world, sem_cls_prob, pred_mask):
            if t.device != self.device:
                raise RuntimeError("parq_amd.SceneTracks: tensors must be on %s, got %s (no CPU fallback)" % (self.device, t.device))
        corners = corners_world.detach().to(torch.float32).contiguous()
        prob = sem_cls_prob.detach().to(torch.float32).contiguous()
        mask = (pred_mask.view(torch.uint8) if pred_mask.dtype == torch.bool else pred_mask).contiguous()
        track_id = torch.empty(B, Q, dtype=torch.int32, device=self.device)
        if B == 0:
            return track_id
        slots = [self._slot(n) for n in names]
        self._grow(len(self._slots))
        seen, waves = {}, []
        for b, s in enumerate(slots):
            k = seen.get(s, 0)
            seen[s] = k + 1
            if k == len(waves):
                waves.append([])
            waves[k].append(b)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            stream = _lib.stream_ptr()
            for wave in waves:
                whole = len(wave) == B
                # a wave that is not the whole batch gathers its scenes (device gathers with host-known indices)
                if whole:
                    c_w, p_w, m_w, t_w, i_w = corners, prob, mask, track_id, iou_out
                else:
                    idx = torch.tensor(wave, dtype=torch.int64).to(self.device, non_blocking=True)
                    c_w, p_w, m_w = corners.index_select(0, idx), prob.index_select(0, idx), mask.index_select(0, idx)
                    t_w = torch.empty(len(wave), Q, dtype=torch.int32, device=self.device)
                    i_w = None if iou_out is None else torch.zeros(len(wave), Q, self.max_tracks, dtype=torch.float32, device=self.device)
                need = lib.parq_tracks_update_workspace_bytes(len(wave), Q, self.max_tracks)
                if self._ws is None or self._ws.numel() < need:
                    self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                arr = (C.c_int32 * len(wave))(*[slots[b] for b in wave])
                _lib.check(lib.parq_tracks_update(C.c_void_p(self._store.data_ptr()), self._store.shape[0], self.max_tracks, arr, len(wave),
                                                  _lib.ptr(c_w), _lib.ptr(p_w), C.c_void_p(m_w.data_ptr()), Q, self.num_classes,
                                                  self.conf_thresh, self.iou_thresh, C.c_void_p(self._ws.data_ptr()), self._ws.numel(),
                                                  C.c_void_p(t_w.data_ptr()), None if i_w is None else _lib.ptr(i_w), stream),
                           "parq_tracks_update")
                self.enqueues += 1
                if not whole:
                    track_id.index_copy_(0, idx, t_w)
                    if iou_out is not None:
                        iou_out.index_copy_(0, idx, i_w)
        return track_id

    # ---- reading ----------------------------------------------------------------------------------------------------------
    def boxes(self, name):
        """Device views of one scene's tracks, nothing copied: {"count" (0-dim int32), "corners" (max_tracks,8,3), "labels"
        (max_tracks) int32, "scores" (max_tracks)}; rows from ``count`` on are unused.  They feed ``parq_amd.draw_boxes(...,
        count=)`` directly (after an ``[None]`` for its batch axis)."""
        v = self._views(self._slots[name])
        return {k: v[k] for k in ("count", "corners", "labels", "scores")}

    def to_host(self, name=None):
        """The tracks as F1Calculator's entries ``[class, corners (8,3) float32, score (np.float32), id]``: a list for one scene,
        {name: list} for all.  The one call that synchronises (one copy of the store)."""
        if name is not None and name not in self._slots:
            raise KeyError(name)
        if self._store is None:
            return {}
        host = self._store[:len(self._slots)].cpu().numpy()
        mt = self.max_tracks
        out = {}
        for n, s in self._slots.items():
            if name is not None and n != name:
                continue
            row = host[s]
            cnt = int(min(max(row[0], 0), mt))
            scores = row[2 + mt:2 + 2 * mt].view(np.float32)
            corners = row[2 + 2 * mt:].view(np.float32).reshape(mt, 8, 3)
            out[n] = [[int(row[2 + t]), corners[t].copy(), scores[t], t] for t in range(cnt)]
        return out[name] if name is not None else out

    def dropped(self):
        """{name: detections that found the scene's store full}.  Synchronises."""
        if self._store is None:
            return {}
        host = self._store[:len(self._slots), 1].cpu().numpy()
        return {n: int(host[s]) for n, s in self._slots.items()}

    def names(self):
        return list(self._slots)

    def reset(self, name=None):
        """Forget every scene, or empty one scene's slot (its name keeps the slot)."""
        if name is None:
            self._slots = {}
            if self._store is not None:
                self._store.zero_()
        elif name in self._slots:
            self._store[self._slots[name], :2].zero_()
