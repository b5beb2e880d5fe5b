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

The evaluator's ground truth can live in a second store: ``update_labelled`` (parq_gt_tracks_update) follows labelled boxes under
the same rule, and ``f1_counts`` (parq_f1_counts, csrc/f1_counts.hip) turns a prediction and a ground-truth store into the
per-class counts of the F1 metrics; their NumPy statements are tests/f1_device_cases.py.  ``average_precision``
(parq_average_precision, csrc/avg_precision.hip) gives AP per IoU threshold and class from the same two stores, a metric the
reference's evaluator does not have; its NumPy statement is tests/average_precision_cases.py.

A stream needs more than the evaluator's rule: ``SceneTracks(lifecycle=True)`` keeps a second device record per scene, the life
(include/parq_hip.h parq_tracks_note, parq_tracks_retire, csrc/track_life.hip): a stable ``uid``, the hit count and the first / last
sighting of every track, noted behind each update, and ``retire`` removes the tracks nobody has seen for too long, so that the
store does not fill up.  Its NumPy statement is tests/track_life_cases.py.  Off (the default) nothing of it exists.
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


def check_labelled_args(corners_world, labels, valid, n_names):
    """Shapes / dtypes of one ground-truth update (ValueError before anything touches the GPU); returns (B, P)."""
    if not (torch.is_tensor(corners_world) and corners_world.ndim == 4 and tuple(corners_world.shape[2:]) == (8, 3)
            and corners_world.is_floating_point()):
        raise ValueError("corners_world must be a floating-point (B, P, 8, 3) tensor, got %s" % (tuple(getattr(corners_world, "shape", ())),))
    B, P = corners_world.shape[:2]
    if not (torch.is_tensor(labels) and tuple(labels.shape) == (B, P) and not labels.is_floating_point() and labels.dtype != torch.bool):
        raise ValueError("labels must be an integer (B, P) tensor for B = %d, P = %d" % (B, P))
    if not (torch.is_tensor(valid) and tuple(valid.shape) == (B, P) and valid.dtype in (torch.bool, torch.uint8)):
        raise ValueError("valid must be a bool or uint8 (B, P) tensor for B = %d, P = %d" % (B, P))
    if n_names != B:
        raise ValueError("%d scene names for a batch of %d scenes" % (n_names, B))
    if not 1 <= P <= MAX_SIDE:
        raise ValueError("P = %d: the store takes 1 to %d labelled boxes per scene" % (P, MAX_SIDE))
    return B, P


def check_life_out(t, what, rows, cols):
    """An output of a life launch (uid_out, hits_out, remap_out): a contiguous int32 (rows, cols) tensor (ValueError otherwise)."""
    if not (torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == (rows, cols) and t.is_contiguous()):
        raise ValueError("%s must be a contiguous int32 (%d, %d) tensor, got %s %s"
                         % (what, rows, cols, getattr(t, "dtype", type(t).__name__), tuple(getattr(t, "shape", ()))))


def check_retire_args(names, min_hits, max_age, tentative_age):
    """The arguments of one retire (ValueError before anything touches the GPU); returns the names as a list."""
    names = list(names)
    if len(set(names)) != len(names):
        twice = sorted({n for n in names if names.count(n) > 1}, key=str)
        raise ValueError("retire: scene %r is listed twice; a scene is retired once per call" % (twice[0],))
    for what, v in (("min_hits", min_hits), ("max_age", max_age), ("tentative_age", tentative_age)):
        if isinstance(v, bool) or not isinstance(v, int) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("retire: %s must be a 32-bit integer, got %r" % (what, v))
    if min_hits < 1:
        raise ValueError("retire: min_hits = %d; a confirmed track has at least one hit (min_hits >= 1)" % min_hits)
    return names


class SceneTracks:
    """A device-resident track store: ``update`` follows the detections of a snippet batch, ``boxes`` / ``to_host`` read the scenes'
    objects.  ``max_tracks`` is the capacity per scene (at most 2048): a detection that would open a track beyond it gets id -2 and
    is counted in ``dropped()`` — the store never overflows silently.  ``num_classes`` counts the background class, which is the
    last one.  ``lifecycle=True`` adds the tracks' life (``retire``, ``life``, ``confirmed``, ``life_to_host``, ``update``'s
    ``uid_out`` / ``hits_out``); without it none of that exists and an update enqueues exactly what it always did.  Nothing here
    synchronises except ``to_host``, ``life_to_host`` and ``dropped``."""

    def __init__(self, max_tracks=512, conf_thresh=0.1, iou_thresh=0.1, num_classes=10, device="cuda", lifecycle=False):
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
        self._visits = {}                      # slot -> update_labelled visits so far (a word of the jitter's key)
        self.enqueues = 0                      # parq_tracks_update / parq_gt_tracks_update calls so far
        self.lifecycle = bool(lifecycle)
        self._life_words = 4 + 4 * max_tracks
        self._life = None                      # (S_cap, life words) int32, with lifecycle only
        self._arange = None
        self.life_enqueues = 0                 # parq_tracks_note / parq_tracks_retire calls so far

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
        if self.lifecycle:
            assert lib.parq_tracks_life_bytes(new_cap, self.max_tracks) == new_cap * self._life_words * 4
            life = torch.zeros(new_cap, self._life_words, dtype=torch.int32, device=self.device)
            if cap:
                life[:cap].copy_(self._life)
            self._life = life

    def _need_life(self, what):
        if not self.lifecycle:
            raise ValueError("%s needs the tracks' life record: construct SceneTracks with lifecycle=True" % what)

    def _life_out(self, t, what, rows, cols):
        """An optional int32 (rows, cols) device tensor that a life launch fills."""
        if t is None:
            return None
        self._need_life(what)
        check_life_out(t, what, rows, cols)
        if t.device != self.device:
            raise RuntimeError("parq_amd.SceneTracks: %s must be on %s, got %s (no CPU fallback)" % (what, self.device, t.device))
        return t

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
    def update(self, scene_names, corners_world, sem_cls_prob, pred_mask, iou_out=None, uid_out=None, hits_out=None):
        """scene_names [B]; corners_world (B,Q,8,3); sem_cls_prob (B,Q,num_classes); pred_mask (B,Q) bool / uint8 -> track_id (B,Q)
        int32 on the device: the track of each detection, -1 for a query that is no detection, -2 for a detection the full store
        could not take.  A name listed k times is processed in k enqueues, each seeing what the previous one left.  ``iou_out``
        (tests): a float32 (B, Q, max_tracks) device tensor that receives the IoU matrices.  With ``lifecycle`` every enqueue is
        followed by parq_tracks_note, and ``uid_out`` / ``hits_out``, int32 (B,Q) device tensors, receive each detection's stable
        id (-1 / -2 as in track_id) and the hits of its track, this one included."""
        names = list(scene_names)
        B, Q = check_tracks_args(corners_world, sem_cls_prob, pred_mask, len(names), self.num_classes)
        if uid_out is not None or hits_out is not None:
            self._need_life("update(uid_out= / hits_out=)")
        if self.device.index is None and corners_world.is_cuda:
            self.device = corners_world.device                    # "cuda": the device of the first batch
        for t in (corners_world, sem_cls_prob, pred_mask):
            if t.device != self.device:
                raise RuntimeError("parq_amd.SceneTracks: tensors must be on %s, got %s (no CPU fallback)" % (self.device, t.device))
        uid_out, hits_out = self._life_out(uid_out, "uid_out", B, Q), self._life_out(hits_out, "hits_out", B, Q)
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
                if self.lifecycle:
                    u_w, h_w = uid_out, hits_out
                    if not whole:
                        u_w = None if uid_out is None else torch.empty(len(wave), Q, dtype=torch.int32, device=self.device)
                        h_w = None if hits_out is None else torch.empty(len(wave), Q, dtype=torch.int32, device=self.device)
                    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
                    _lib.check(lib.parq_tracks_note(C.c_void_p(self._store.data_ptr()), C.c_void_p(self._life.data_ptr()),
                                                    self._store.shape[0], self.max_tracks, arr, len(wave), C.c_void_p(t_w.data_ptr()), Q,
                                                    dp(u_w), dp(h_w), stream), "parq_tracks_note")
                    self.life_enqueues += 1
                    if not whole:
                        if uid_out is not None:
                            uid_out.index_copy_(0, idx, u_w)
                        if hits_out is not None:
                            hits_out.index_copy_(0, idx, h_w)
                if not whole:
                    track_id.index_copy_(0, idx, t_w)
                    if iou_out is not None:
                        iou_out.index_copy_(0, idx, i_w)
        return track_id

    @torch.no_grad()
    def update_labelled(self, scene_names, corners_world, labels, valid, seed=0, iou_out=None):
        """The evaluator's ground-truth side (include/parq_hip.h parq_gt_tracks_update): scene_names [B]; corners_world (B,P,8,3);
        labels (B,P) integers; valid (B,P) bool / uint8.  Every valid row is a detection of score 1 with its own label, its corners
        moved by the hashed jitter of (seed, slot, visit, rank among the valid rows); the rest is ``update``'s rule.  A name listed
        k times is processed in k enqueues, and each counts as a visit of its scene.  Returns nothing and does not synchronise.
        ``iou_out`` (tests): a float32 (B, P, max_tracks) device tensor that receives the IoU matrices."""
        if self.lifecycle:
            raise ValueError("update_labelled: ground truth has no life; feed a SceneTracks built without lifecycle=True")
        names = list(scene_names)
        B, P = check_labelled_args(corners_world, labels, valid, len(names))
        if self.device.index is None and corners_world.is_cuda:
            self.device = corners_world.device
        for t in (corners_world, labels, valid):
            if t.device != self.device:
                raise RuntimeError("parq_amd.SceneTracks: tensors must be on %s, got %s (no CPU fallback)" % (self.device, t.device))
        if B == 0:
            return
        corners = corners_world.detach().to(torch.float32).contiguous()
        lab = labels.to(torch.int32).contiguous()
        ok = (valid.view(torch.uint8) if valid.dtype == torch.bool else valid).contiguous()
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
                if whole:
                    c_w, l_w, v_w, i_w = corners, lab, ok, iou_out
                else:
                    idx = torch.tensor(wave, dtype=torch.int64).to(self.device, non_blocking=True)
                    c_w, l_w, v_w = corners.index_select(0, idx), lab.index_select(0, idx), ok.index_select(0, idx)
                    i_w = None if iou_out is None else torch.zeros(len(wave), P, self.max_tracks, dtype=torch.float32, device=self.device)
                need = lib.parq_gt_tracks_update_workspace_bytes(len(wave), P, self.max_tracks)
                if self._ws is None or self._ws.numel() < need:
                    self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
                arr = (C.c_int32 * len(wave))(*[slots[b] for b in wave])
                visits = (C.c_int32 * len(wave))(*[self._visits.get(slots[b], 0) for b in wave])
                _lib.check(lib.parq_gt_tracks_update(C.c_void_p(self._store.data_ptr()), self._store.shape[0], self.max_tracks, arr, visits,
                                                     len(wave), _lib.ptr(c_w), C.c_void_p(l_w.data_ptr()), C.c_void_p(v_w.data_ptr()), P,
                                                     self.iou_thresh, int(seed) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(self._ws.data_ptr()),
                                                     self._ws.numel(), None if i_w is None else _lib.ptr(i_w), stream),
                           "parq_gt_tracks_update")
                self.enqueues += 1
                for b in wave:
                    self._visits[slots[b]] = self._visits.get(slots[b], 0) + 1
                if not whole and iou_out is not None:
                    iou_out.index_copy_(0, idx, i_w)

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
        """Forget every scene, or empty one scene's slot (its name keeps the slot).  A slot's life goes with its count: its clock and
        its uids start from 0 again."""
        if name is None:
            self._slots = {}
            self._visits = {}
            if self._store is not None:
                self._store.zero_()
            if self._life is not None:
                self._life.zero_()
        elif name in self._slots:
            self._visits.pop(self._slots[name], None)
            self._store[self._slots[name], :2].zero_()
            if self._life is not None:
                self._life[self._slots[name], :4].zero_()

    # ---- the tracks' life (lifecycle=True) -------------------------------------------------------------------------------------
    @torch.no_grad()
    def retire(self, names=None, min_hits=3, max_age=30, tentative_age=1, remap_out=None):
        """Remove the tracks nobody has seen for too long (include/parq_hip.h parq_tracks_retire) from the scenes ``names`` (None:
        every scene, in ``names()`` order).  A track's age is the number of its scene's updates since it was last matched; a track
        with at least ``min_hits`` hits is confirmed and goes when its age exceeds ``max_age``, any other when it exceeds
        ``tentative_age`` (negative: never).  The kept tracks move up in their order, so ``track_id``, a position, changes here and
        ``track_uid`` does not; ``remap_out``, an int32 (len(names), max_tracks) device tensor, receives each old position's new one
        (-1: removed or unused).  One enqueue; does not synchronise."""
        self._need_life("retire")
        names = check_retire_args(self.names() if names is None else names, min_hits, max_age, tentative_age)
        for n in names:
            if n not in self._slots:
                raise KeyError(n)
        if remap_out is not None:
            self._life_out(remap_out, "remap_out", len(names), self.max_tracks)
        if not names:
            return
        lib = _lib.load()
        arr = (C.c_int32 * len(names))(*[self._slots[n] for n in names])
        with torch.cuda.device(self.device):
            _lib.check(lib.parq_tracks_retire(C.c_void_p(self._store.data_ptr()), C.c_void_p(self._life.data_ptr()), self._store.shape[0],
                                              self.max_tracks, arr, len(names), min_hits, max_age, tentative_age,
                                              None if remap_out is None else C.c_void_p(remap_out.data_ptr()), _lib.stream_ptr()),
                       "parq_tracks_retire")
        self.life_enqueues += 1

    def life(self, name):
        """Device views of one scene's life, nothing copied: {"step" (0-dim int32: the scene's updates so far), "uid", "hits",
        "first", "last" (max_tracks) int32}; rows from the scene's ``count`` on are unused."""
        self._need_life("life")
        mt = self.max_tracks
        row = self._life[self._slots[name]]
        return {"step": row[0], "uid": row[4:4 + mt], "hits": row[4 + mt:4 + 2 * mt], "first": row[4 + 2 * mt:4 + 3 * mt],
                "last": row[4 + 3 * mt:4 + 4 * mt]}

    def confirmed(self, name, min_hits=3):
        """(max_tracks,) bool on the device: the scene's tracks with at least ``min_hits`` hits; rows from ``count`` on are false.
        It is ``parq_amd.draw_boxes``'s ``keep=`` for ``boxes(name)`` (after an ``[None]``).  Does not synchronise."""
        self._need_life("confirmed")
        if self._arange is None or self._arange.device != self.device:
            self._arange = torch.arange(self.max_tracks, dtype=torch.int32, device=self.device)
        return (self.life(name)["hits"] >= min_hits) & (self._arange < self._views(self._slots[name])["count"])

    def life_to_host(self, name=None):
        """``to_host`` with each track's life: entries ``[class, corners (8,3) float32, score (np.float32), id, uid, hits, first,
        last]``, a list for one scene, {name: list} for all.  Synchronises (one copy of the store and one of the life)."""
        self._need_life("life_to_host")
        tracks = self.to_host(name)
        if self._life is None:
            return tracks
        host = self._life[:len(self._slots)].cpu().numpy()
        mt = self.max_tracks
        for n, entries in ([(name, tracks)] if name is not None else tracks.items()):
            row = host[self._slots[n]]
            for e in entries:
                e.extend(int(row[4 + f * mt + e[3]]) for f in range(4))
        return tracks


F1_MAX_THRESHOLDS = 8


def f1_counts(pred_tracks, gt_tracks, thresholds, num_classes=9, best_iou_out=None, out=None):
    """The evaluator's end-of-epoch counts from two ``SceneTracks`` with the same scenes in the same slots (include/parq_hip.h
    parq_f1_counts): (counts (2 + T, num_classes) int64, invalid (2) int64), both on the device.  counts[0] / counts[1]: the
    ground-truth / prediction tracks per class, counts[2 + t]: the ground-truth tracks whose best same-class prediction has
    IoU > thresholds[t]; invalid: tracks of either side with a label outside [0, num_classes).  Only enqueues.
    ``best_iou_out`` (tests): a float64 (scenes, gt_tracks.max_tracks) device tensor.  ``out``: an int64 device tensor of at least
    (2 + T) * num_classes + 2 elements to place both results in (counts first), for callers that copy them back with more."""
    thr = [float(t) for t in thresholds]
    T = len(thr)
    if not 1 <= T <= F1_MAX_THRESHOLDS:
        raise ValueError("f1_counts takes 1 to %d thresholds, got %d" % (F1_MAX_THRESHOLDS, T))
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= 32:
        raise ValueError("num_classes must be an integer in [1, 32], got %r" % (num_classes,))
    if not (isinstance(pred_tracks, SceneTracks) and isinstance(gt_tracks, SceneTracks)):
        raise TypeError("f1_counts takes two SceneTracks")
    if pred_tracks._slots != gt_tracks._slots:
        raise ValueError("f1_counts: the two stores do not hold the same scenes in the same slots (feed both with the same names)")
    if pred_tracks.device != gt_tracks.device:
        raise RuntimeError("f1_counts: the stores are on %s and %s" % (pred_tracks.device, gt_tracks.device))
    dev = pred_tracks.device
    S = len(pred_tracks._slots)
    n = (2 + T) * num_classes
    if out is None:
        out = torch.empty(n + 2, dtype=torch.int64, device=dev)
    assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= n + 2
    counts, invalid = out[:n].view(2 + T, num_classes), out[n:n + 2]
    if S == 0:
        out[:n + 2].zero_()
        return counts, invalid
    if best_iou_out is not None:
        assert best_iou_out.is_cuda and best_iou_out.dtype == torch.float64 and best_iou_out.is_contiguous()
        assert tuple(best_iou_out.shape) == (S, gt_tracks.max_tracks), tuple(best_iou_out.shape)
    lib = _lib.load()
    with torch.cuda.device(dev):
        need = lib.parq_f1_counts_workspace_bytes(S, gt_tracks.max_tracks, T, num_classes)
        if gt_tracks._ws is None or gt_tracks._ws.numel() < need:
            gt_tracks._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        ws = gt_tracks._ws
        _lib.check(lib.parq_f1_counts(C.c_void_p(pred_tracks._store.data_ptr()), pred_tracks.max_tracks, C.c_void_p(gt_tracks._store.data_ptr()),
                                      gt_tracks.max_tracks, S, (C.c_double * T)(*thr), T, num_classes, C.c_void_p(ws.data_ptr()), ws.numel(),
                                      C.c_void_p(counts.data_ptr()), C.c_void_p(invalid.data_ptr()),
                                      None if best_iou_out is None else C.c_void_p(best_iou_out.data_ptr()), _lib.stream_ptr()),
                   "parq_f1_counts")
    return counts, invalid


AP_MAX_POSITIONS = 1 << 20  # scenes x prediction capacity that parq_average_precision ranks in one call


def check_average_precision_args(pred_tracks, gt_tracks, thresholds, num_classes):
    """The arguments of ``average_precision`` (an error before anything touches the GPU); returns (thresholds as floats, scenes)."""
    thr = [float(t) for t in thresholds]
    if not 1 <= len(thr) <= F1_MAX_THRESHOLDS:
        raise ValueError("average_precision takes 1 to %d thresholds, got %d" % (F1_MAX_THRESHOLDS, len(thr)))
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= 32:
        raise ValueError("num_classes must be an integer in [1, 32], got %r" % (num_classes,))
    if not (isinstance(pred_tracks, SceneTracks) and isinstance(gt_tracks, SceneTracks)):
        raise TypeError("average_precision takes two SceneTracks")
    if pred_tracks._slots != gt_tracks._slots:
        raise ValueError("average_precision: the two stores do not hold the same scenes in the same slots (feed both with the same names)")
    if pred_tracks.device != gt_tracks.device:
        raise RuntimeError("average_precision: the stores are on %s and %s" % (pred_tracks.device, gt_tracks.device))
    S = len(pred_tracks._slots)
    if S * pred_tracks.max_tracks > AP_MAX_POSITIONS:
        raise ValueError("average_precision: %d scenes x %d tracks; at most %d positions are ranked" % (S, pred_tracks.max_tracks, AP_MAX_POSITIONS))
    return thr, S


def average_precision(pred_tracks, gt_tracks, thresholds, num_classes=9, curves=False, out=None):
    """Average precision per (IoU threshold, class) from two ``SceneTracks`` with the same scenes in the same slots (include/parq_hip.h
    parq_average_precision, where the rule is stated in full): (ap (T, num_classes) float64, counts (2, num_classes) int64, invalid
    (2) int64), all on the device.  counts[0] / counts[1]: the ground-truth / ranked prediction tracks per class; invalid: tracks
    that are not ranked (a label outside [0, num_classes), or a NaN score on the prediction side).  Only enqueues.  The reference's
    evaluator has no AP: this is not one of its numbers.  The stores hold the tracks selected at the tracker's confidence threshold,
    so a curve ends there.  ``curves=True`` appends a dict of the curve's parts: "order" (N) int32, "class_start" (num_classes + 1)
    int32, "cum_tp" (T, N) int32, "pred_best" (scenes, pred max_tracks) float64, "pred_target" (the same shape) int32, with
    N = scenes * pred max_tracks.  ``out``: an int64 device tensor of at least (T + 2) * num_classes + 2 elements to place the
    three results in (ap first, its float64 bits), for callers that copy them back with more."""
    thr, S = check_average_precision_args(pred_tracks, gt_tracks, thresholds, num_classes)
    T, K = len(thr), num_classes
    dev = pred_tracks.device
    n = (T + 2) * K
    if out is None:
        out = torch.empty(n + 2, dtype=torch.int64, device=dev)
    assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() >= n + 2
    ap, counts, invalid = out[:T * K].view(torch.float64).view(T, K), out[T * K:n].view(2, K), out[n:n + 2]
    N = S * pred_tracks.max_tracks
    extra = None
    if curves:
        extra = {"order": torch.empty(N, dtype=torch.int32, device=dev), "class_start": torch.empty(K + 1, dtype=torch.int32, device=dev),
                 "cum_tp": torch.empty(T, N, dtype=torch.int32, device=dev),
                 "pred_best": torch.zeros(S, pred_tracks.max_tracks, dtype=torch.float64, device=dev),
                 "pred_target": torch.full((S, pred_tracks.max_tracks), -1, dtype=torch.int32, device=dev)}
    if S == 0:
        out[:n + 2].zero_()
        if curves:
            extra["class_start"].zero_()
        return (ap, counts, invalid, extra) if curves else (ap, counts, invalid)
    lib = _lib.load()
    with torch.cuda.device(dev):
        need = lib.parq_average_precision_workspace_bytes(S, pred_tracks.max_tracks, gt_tracks.max_tracks, T, K)
        if gt_tracks._ws is None or gt_tracks._ws.numel() < need:
            gt_tracks._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        ws = gt_tracks._ws
        opt = [C.c_void_p(extra[k].data_ptr()) if curves else None for k in ("order", "class_start", "cum_tp", "pred_best", "pred_target")]
        _lib.check(lib.parq_average_precision(C.c_void_p(pred_tracks._store.data_ptr()), pred_tracks.max_tracks,
                                              C.c_void_p(gt_tracks._store.data_ptr()), gt_tracks.max_tracks, S, (C.c_double * T)(*thr), T, K,
                                              C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(ap.data_ptr()), C.c_void_p(counts.data_ptr()),
                                              C.c_void_p(invalid.data_ptr()), *opt, _lib.stream_ptr()),
                   "parq_average_precision")
    return (ap, counts, invalid, extra) if curves else (ap, counts, invalid)
