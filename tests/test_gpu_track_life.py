"""GPU tier of the tracks' life: parq_tracks_note and parq_tracks_retire (csrc/track_life.hip) against their NumPy statements
(tests/track_life_cases.py) bit for bit, behind the real parq_tracks_update; then SceneTracks(lifecycle=True) on the unbounded
stream, the promise that nothing but life_to_host synchronises, the untouched default, and confirmed() as draw_boxes' keep=."""
import ctypes as C

import numpy as np
import pytest
import torch

import f1_device_cases as F
import scene_tracks_cases as T
import track_life_cases as L
from gpu_util import lib
from oracle.make_golden import _yaw_box_corners
from parq_amd import Pose, SceneTracks, _lib, draw_boxes

pytestmark = pytest.mark.gpu

CANARY = -77


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw_update(store, mt, slots, st, conf=0.1, iou=0.1):
    """The real parq_tracks_update on a raw store; returns track_id (B,Q) on the device."""
    l = lib()
    B, Q = st["corners"].shape[:2]
    corners, prob, mask = cuda(st["corners"]), cuda(st["prob"]), cuda(st["mask"].astype(np.uint8))
    need = l.parq_tracks_update_workspace_bytes(B, Q, mt)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    tid = torch.full((B, Q), CANARY, dtype=torch.int32, device="cuda")
    rc = l.parq_tracks_update(vp(store), store.shape[0], mt, (C.c_int32 * B)(*slots), B, vp(corners), vp(prob), vp(mask), Q, st["prob"].shape[2],
                              conf, iou, vp(ws), need, vp(tid), None, _lib.stream_ptr())
    assert rc == 0, l.parq_last_error()
    return tid


def raw_note(store, life, mt, slots, tid, outs=True, expect=0):
    l = lib()
    B, Q = tid.shape
    uid = torch.full((B, Q), CANARY, dtype=torch.int32, device="cuda") if outs else None
    hits = torch.full((B, Q), CANARY, dtype=torch.int32, device="cuda") if outs else None
    rc = l.parq_tracks_note(vp(store), vp(life), store.shape[0], mt, (C.c_int32 * len(slots))(*slots), len(slots), vp(tid), Q, vp(uid), vp(hits),
                            _lib.stream_ptr())
    assert rc == expect, l.parq_last_error()
    return uid, hits


def raw_retire(store, life, mt, slots, rule, remap=True, expect=0):
    l = lib()
    out = torch.full((len(slots), mt), CANARY, dtype=torch.int32, device="cuda") if remap else None
    rc = l.parq_tracks_retire(vp(store), vp(life), store.shape[0], mt, (C.c_int32 * len(slots))(*slots), len(slots), rule["min_hits"],
                              rule["max_age"], rule["tentative_age"], vp(out), _lib.stream_ptr())
    assert rc == expect, l.parq_last_error()
    return out


def fresh(S_cap, mt, used):
    """A zeroed store and life of S_cap slots, the slots not in `used` filled with a canary."""
    store = torch.zeros(S_cap, L.store_words(mt), dtype=torch.int32, device="cuda")
    life = torch.zeros(S_cap, L.life_words(mt), dtype=torch.int32, device="cuda")
    guard = [s for s in range(S_cap) if s not in used]
    store[guard] = CANARY
    life[guard] = CANARY
    return store, life


# max_tracks {1, 63, 64, 65, 129, 512, 2048} x Q {1, 64, 65, 257} x B {1, 3, one above a slot chunk of 64}, every value at least once;
# `world` boxes per scene: more than max_tracks where the store is to fill up and answer -2
NOTE_CASES = [dict(mt=1, Q=1, B=1, steps=3, world=2, p=0.6, full=True), dict(mt=1, Q=64, B=3, steps=2, world=70, p=0.6, full=True),
              dict(mt=63, Q=64, B=3, steps=3, world=80, p=0.6, full=True), dict(mt=64, Q=65, B=1, steps=3, world=100, p=0.6, full=True),
              dict(mt=65, Q=257, B=3, steps=2, world=300, p=0.6, full=True), dict(mt=129, Q=64, B=66, steps=5, world=160, p=0.9, full=True),
              dict(mt=512, Q=257, B=1, steps=4, world=700, p=0.9, full=True), dict(mt=2048, Q=257, B=3, steps=5, world=2304, p=0.95, full=False),
              dict(mt=2048, Q=1, B=1, steps=2, world=2, p=0.6, full=False)]


@pytest.mark.parametrize("c", NOTE_CASES, ids=lambda c: "mt%d-Q%d-B%d" % (c["mt"], c["Q"], c["B"]))
def test_note_equals_the_statement_after_every_step(c):
    mt, Q, B = c["mt"], c["Q"], c["B"]
    slots = [2 * b + 1 for b in reversed(range(B))]                          # non-contiguous, not in order
    store, life = fresh(2 * B + 1, mt, slots)
    want_life = life.cpu().numpy()
    births = overflow = 0
    steps = L.scatter_steps(100 + mt + Q, B, Q, c["steps"], c["world"], c["p"])
    distinct = [len(set(np.concatenate([st["objects"][b] for st in steps]).tolist()) - {-1}) for b in range(B)]
    for k, st in enumerate(steps):
        tid = raw_update(store, mt, slots, st)
        before = store.clone()
        uid, hits = raw_note(store, life, mt, slots, tid)
        assert torch.equal(store, before), k                                 # the store is read only
        host, ids, uid, hits = store.cpu().numpy(), tid.cpu().numpy(), uid.cpu().numpy(), hits.cpu().numpy()
        for b, s in enumerate(slots):
            known = int(want_life[s, 1])
            want_uid, want_hits = L.note_ref(host[s], want_life[s], ids[b])
            assert np.array_equal(uid[b], want_uid) and np.array_equal(hits[b], want_hits), (k, b)
            births += int(want_life[s, 1]) - known
            overflow += int((ids[b] == -2).sum())
        assert np.array_equal(life.cpu().numpy(), want_life), k               # every word, the guard slots included
    # the boxes are far apart, so a track is a world box: the case did what it was built for (c["full"]: some store filled up)
    assert births == sum(min(d, mt) for d in distinct) > 0 and (overflow > 0) == any(d > mt for d in distinct) == c["full"], (births, overflow)


def test_note_on_a_full_store_and_without_outputs():
    st = T.overflow_step()                                                   # 12 births into a store of 8: ids 0..7 and four -2
    mt = 8
    store, life = fresh(2, mt, [0])
    want_life = life.cpu().numpy()
    for k in range(2):
        st = dict(st, corners=st["corners"] + np.float32(0.02 * k))         # the second visit 2 cm away: eight matches, four more -2
        tid = raw_update(store, mt, [0], st)
        uid, hits = raw_note(store, life, mt, [0], tid)
        ids = tid.cpu().numpy()
        want_uid, want_hits = L.note_ref(store.cpu().numpy()[0], want_life[0], ids[0])
        assert np.array_equal(uid.cpu().numpy()[0], want_uid) and np.array_equal(hits.cpu().numpy()[0], want_hits), k
        assert np.array_equal(life.cpu().numpy(), want_life), k
        assert sorted(want_uid[ids[0] != -1].tolist()) == [-2] * 4 + list(range(8)) and int((ids == -2).sum()) == 4, k
    assert want_life[0, :4].tolist() == [2, 8, 8, 0]
    # NULL outputs: the life is written all the same
    tid = raw_update(store, mt, [0], st)
    assert raw_note(store, life, mt, [0], tid, outs=False) == (None, None)
    L.note_ref(store.cpu().numpy()[0], want_life[0], tid.cpu().numpy()[0])
    assert np.array_equal(life.cpu().numpy(), want_life) and want_life[0, 0] == 3


@pytest.mark.parametrize("mt", [1, 63, 64, 65, 129, 512, 2048])
def test_retire_equals_the_statement_on_every_drop_pattern(mt):
    """One launch: a slot per drop pattern, slots non-contiguous and not in order, random words in every row."""
    B = len(L.DROP_PATTERNS)
    slots = [2 * b + 1 for b in reversed(range(B))]
    S_cap = 2 * B + 1
    store_h = np.full((S_cap, L.store_words(mt)), CANARY, np.int32)
    life_h = np.full((S_cap, L.life_words(mt)), CANARY, np.int32)
    drops = []
    for b, pattern in enumerate(L.DROP_PATTERNS):
        store_h[slots[b]], life_h[slots[b]], drop = L.retire_case(mt, pattern, 1000 * mt + b)
        drops.append(drop)
    store, life = cuda(store_h), cuda(life_h)
    remap = raw_retire(store, life, mt, slots, L.RETIRE_RULE).cpu().numpy()
    got_s, got_l = store.cpu().numpy(), life.cpu().numpy()
    want_s, want_l = store_h.copy(), life_h.copy()
    for b, pattern in enumerate(L.DROP_PATTERNS):
        s = slots[b]
        want_remap = L.retire_ref(want_s[s], want_l[s], **L.RETIRE_RULE)
        n, m = int(store_h[s, 0]), int(want_s[s, 0])
        assert m == n - int(drops[b].sum()) and np.array_equal(want_remap[:n] < 0, drops[b]), (pattern, n, m)   # the pattern is what it says
        assert np.array_equal(remap[b], want_remap), pattern
        assert np.array_equal(got_s[s], want_s[s]) and np.array_equal(got_l[s], want_l[s]), pattern
        # rows from m on are the input's: labels, scores, corners, and the four arrays of the life
        for words, before, width in ((got_s[s, 2:2 + 2 * mt].reshape(2, mt), store_h[s, 2:2 + 2 * mt].reshape(2, mt), 1),
                                     (got_l[s, 4:].reshape(4, mt), life_h[s, 4:].reshape(4, mt), 1)):
            assert np.array_equal(words[:, m:], before[:, m:]), pattern
        assert np.array_equal(got_s[s, 2 + 2 * mt + 24 * m:], store_h[s, 2 + 2 * mt + 24 * m:]), pattern
        assert got_s[s, 1] == 7 and got_l[s, 0] == 50 and got_l[s, 2] == 1000 and got_l[s, 3] == 3 + (n - m), pattern
    assert np.array_equal(got_s, want_s) and np.array_equal(got_l, want_l)    # the guard slots included
    # a second retire at once removes nothing more and moves nothing; NULL remap_out is taken
    assert raw_retire(store, life, mt, slots, L.RETIRE_RULE, remap=False) is None
    assert np.array_equal(store.cpu().numpy(), want_s) and np.array_equal(life.cpu().numpy(), want_l)


def statement_store(words, mt):
    view = L.store_fields(words, mt)
    view.update(count=int(words[0]), dropped=int(words[1]))
    return view


def test_a_retired_store_feeds_the_update_and_the_counts_unchanged():
    """12 far-apart tracks, every second one aged out by hand, retired; then the unchanged parq_tracks_update sees the same boxes
    2 cm away (six matches, six births) and parq_f1_counts counts the store against a ground truth: both equal their own statements
    on the compacted store."""
    mt = 16
    st = T.overflow_step()
    store, life = fresh(1, mt, [0])
    raw_note(store, life, mt, [0], raw_update(store, mt, [0], st))
    life[0, 4 + 3 * mt + 1:4 + 3 * mt + 12:2] = -10                           # last of tracks 1, 3, .., 11
    want_s, want_l = store.cpu().numpy(), life.cpu().numpy()
    rule = dict(min_hits=1, max_age=2, tentative_age=0)
    remap = raw_retire(store, life, mt, [0], rule).cpu().numpy()
    assert np.array_equal(remap[0], L.retire_ref(want_s[0], want_l[0], **rule)) and remap[0, :12].tolist() == [0, -1, 1, -1, 2, -1, 3, -1, 4, -1, 5, -1]
    assert np.array_equal(store.cpu().numpy(), want_s) and np.array_equal(life.cpu().numpy(), want_l) and want_s[0, 0] == 6
    moved = dict(st, corners=st["corners"] + np.float32(0.02))
    tid = raw_update(store, mt, [0], moved)
    uid, hits = raw_note(store, life, mt, [0], tid)
    want_tid, want_uid, want_hits = L.slot_step(want_s[0], want_l[0], moved["corners"][0], moved["prob"][0], moved["mask"][0], 0.1)
    assert np.array_equal(tid.cpu().numpy()[0], want_tid) and sorted(want_tid[want_tid >= 0].tolist()) == list(range(12))
    assert np.array_equal(uid.cpu().numpy()[0], want_uid) and np.array_equal(hits.cpu().numpy()[0], want_hits)
    assert sorted(want_uid[want_tid >= 0].tolist()) == [0, 2, 4, 6, 8, 10] + list(range(12, 18)) and sorted(want_hits.tolist())[-6:] == [2] * 6
    assert np.array_equal(store.cpu().numpy(), want_s) and np.array_equal(life.cpu().numpy(), want_l)
    # the counts: this store as the prediction, the twelve boxes as the ground truth
    gt, _ = fresh(1, mt, [0])
    raw_update(gt, mt, [0], st)
    l = lib()
    K, thr = F.K_CARE, F.THRESHOLDS
    need = l.parq_f1_counts_workspace_bytes(1, mt, len(thr), K)
    ws = torch.zeros(max(need, 16), dtype=torch.uint8, device="cuda")
    counts = torch.full((2 + len(thr), K), CANARY, dtype=torch.int64, device="cuda")
    invalid = torch.full((2,), CANARY, dtype=torch.int64, device="cuda")
    best = torch.full((1, mt), -1.0, dtype=torch.float64, device="cuda")
    rc = l.parq_f1_counts(vp(store), mt, vp(gt), mt, 1, (C.c_double * len(thr))(*thr), len(thr), K, vp(ws), need, vp(counts), vp(invalid), vp(best),
                          _lib.stream_ptr())
    assert rc == 0, l.parq_last_error()
    gt_h = gt.cpu().numpy()
    want_counts, want_invalid, want_best = F.counts_statement([statement_store(want_s[0], mt)], [statement_store(gt_h[0], mt)])
    assert np.array_equal(counts.cpu().numpy(), want_counts) and np.array_equal(invalid.cpu().numpy(), want_invalid)
    assert np.array_equal(best.cpu().numpy()[0, :12], want_best[0]) and want_counts[1].sum() == 12 and want_counts[2].sum() >= 6


def test_invalid_slots_are_left_untouched_and_refused_calls_write_nothing():
    mt, Q = 8, 6
    slots = [4, 0, 3, 1, 2, 5]                                               # a count above the capacity, known > count, a negative step,
    store, life = fresh(6, mt, slots)                                        # a good one, an update not yet noted (good for note, bad for
    store[:, 0] = torch.tensor([5, 4, 4, 4, 9, -1], dtype=torch.int32)       # retire), a negative count.  These lines are by slot
    life[:, :4] = torch.tensor([[3, 6, 5, 0], [3, 4, 4, 0], [3, 2, 2, 0], [-1, 4, 4, 0], [3, 4, 4, 0], [3, 0, 0, 0]], dtype=torch.int32)
    life[:, 4:4 + mt] = torch.arange(mt, dtype=torch.int32)                  # uids 0.., no hits yet, first = last = 0
    tid = cuda(np.array([[0, 1, -1, -2, 7, 3]] * 6, np.int32))
    before_s, before_l = store.cpu().numpy(), life.cpu().numpy()
    uid, hits = raw_note(store, life, mt, slots, tid)
    want_l = before_l.copy()
    uid, hits = uid.cpu().numpy(), hits.cpu().numpy()
    for b, s in enumerate(slots):
        want_uid, want_hits = L.note_ref(before_s[s], want_l[s], tid.cpu().numpy()[b])
        assert np.array_equal(uid[b], want_uid) and np.array_equal(hits[b], want_hits), b
        if b in (0, 1, 2, 5):
            assert (uid[b] == -1).all() and (hits[b] == 0).all() and np.array_equal(want_l[s], before_l[s]), b
    assert uid[3].tolist() == [0, 1, -1, -2, -1, 3] and hits[3].tolist() == [1, 1, 0, 0, 0, 1]
    assert uid[4].tolist() == [0, 1, -1, -2, -1, 3] and want_l[2, :4].tolist() == [4, 4, 4, 0]        # slot 2: two births, uids 2 and 3
    assert np.array_equal(store.cpu().numpy(), before_s) and np.array_equal(life.cpu().numpy(), want_l)
    # retire: put slot 2 back to "not yet noted"; only slot 1 is taken
    life[2, :4] = torch.tensor([3, 2, 2, 0], dtype=torch.int32)
    before_l = life.cpu().numpy()
    want_s, want_l = before_s.copy(), before_l.copy()
    rule = dict(min_hits=2, max_age=0, tentative_age=0)
    remap = raw_retire(store, life, mt, slots, rule).cpu().numpy()
    for b, s in enumerate(slots):
        assert np.array_equal(remap[b], L.retire_ref(want_s[s], want_l[s], **rule)), b
        if b != 3:
            assert (remap[b] == -1).all() and np.array_equal(want_s[s], before_s[s]) and np.array_equal(want_l[s], before_l[s]), b
    assert remap[3].tolist() == [0, 1, -1, 2, -1, -1, -1, -1] and want_s[1, 0] == 3 and want_l[1, :4].tolist() == [4, 3, 4, 1]
    assert np.array_equal(store.cpu().numpy(), want_s) and np.array_equal(life.cpu().numpy(), want_l)
    # refused calls: nothing is launched, so outputs preset to a fill keep it and store and life keep their bytes
    l = lib()
    for bad in ([1, 1], [0, 6], [-1, 0]):                                    # listed twice, beyond the store's 6 slots, negative
        uid, hits = raw_note(store, life, mt, bad, tid[:2].contiguous(), expect=1)
        remap = raw_retire(store, life, mt, bad, rule, expect=1)
        assert b"parq_tracks_retire" in l.parq_last_error()
        assert bool((uid == CANARY).all()) and bool((hits == CANARY).all()) and bool((remap == CANARY).all()), bad
    remap = raw_retire(store, life, mt, [1], dict(rule, min_hits=0), expect=1)
    assert bool((remap == CANARY).all())
    assert np.array_equal(store.cpu().numpy(), want_s) and np.array_equal(life.cpu().numpy(), want_l)


def test_the_unbounded_stream_through_scene_tracks():
    c = L.STREAM
    steps = L.stream_steps()
    want_plain, want = L.run_stream(retire=False), L.run_stream(retire=True)
    plain = SceneTracks(max_tracks=c["max_tracks"], conf_thresh=c["conf"])
    tracks = SceneTracks(max_tracks=c["max_tracks"], conf_thresh=c["conf"], lifecycle=True)
    uid = torch.empty(1, c["Q"], dtype=torch.int32, device="cuda")
    ids, plain_ids, uids, counts = [], [], {}, []
    for st in steps:
        args = (st["scenes"], cuda(st["corners"]), cuda(st["prob"]), cuda(st["mask"]))
        plain_ids.append(plain.update(*args))
        ids.append(tracks.update(*args, uid_out=uid))
        counts.append(tracks.boxes("stream")["count"].clone())
        for j, q in zip(st["objects"], st["queries"]):
            uids.setdefault(j, []).append(uid[0, q].clone())
        tracks.retire(**c["retire"])
    assert all(np.array_equal(a.cpu().numpy()[0], b) for a, b in zip(plain_ids, want_plain["ids"]))
    assert plain.dropped() == {"stream": want_plain["dropped"]} and want_plain["dropped"] > 0
    assert all(np.array_equal(a.cpu().numpy()[0], b) for a, b in zip(ids, want["ids"]))
    assert [int(x) for x in counts] == want["counts"] and max(want["counts"]) <= c["max_tracks"]
    assert tracks.dropped() == {"stream": 0} and not any(bool((a == -2).any()) for a in ids)
    got_uids = {j: {int(u) for u in us} for j, us in uids.items()}
    assert got_uids == want["uids"] and sorted(next(iter(u)) for u in got_uids.values()) == list(range(c["objects"]))
    assert np.array_equal(tracks._store[0].cpu().numpy(), want["store"]) and np.array_equal(tracks._life[0].cpu().numpy(), want["life"])
    assert tracks.enqueues == len(steps) and tracks.life_enqueues == 2 * len(steps) and plain.life_enqueues == 0
    host = tracks.life_to_host("stream")
    F_ = L.life_fields(want["life"])
    assert [e[3:] for e in host] == [[t] + [int(F_[k][t]) for k in ("uid", "hits", "first", "last")] for t in range(int(want["store"][0]))]
    assert tracks.life_to_host()["stream"][0][4] == host[0][4] and len(host) == 3
    tracks.reset("stream")
    assert tracks._life[0, :4].tolist() == [0, 0, 0, 0] and tracks.life_to_host("stream") == []


def test_a_name_listed_twice_is_noted_wave_by_wave():
    """names a, b, a: two enqueues of the update, a note behind each, outputs through the partial wave's gather and scatter."""
    mt, Q = 16, 8
    steps = L.scatter_steps(7, 3, Q, 3, 10, p_det=0.8)
    tracks = SceneTracks(max_tracks=mt, lifecycle=True)
    words = {n: (np.zeros(L.store_words(mt), np.int32), np.zeros(L.life_words(mt), np.int32)) for n in "ab"}
    for k, st in enumerate(steps):
        uid = torch.full((3, Q), CANARY, dtype=torch.int32, device="cuda")
        hits = torch.full((3, Q), CANARY, dtype=torch.int32, device="cuda")
        tid = tracks.update(["a", "b", "a"], cuda(st["corners"]), cuda(st["prob"]), cuda(st["mask"]), uid_out=uid, hits_out=hits)
        for b, name in ((0, "a"), (1, "b"), (2, "a")):                        # the order the waves see them in
            want = L.slot_step(words[name][0], words[name][1], st["corners"][b], st["prob"][b], st["mask"][b], tracks.conf_thresh)
            for got, w in zip((tid, uid, hits), want):
                assert np.array_equal(got[b].cpu().numpy(), w), (k, b)
        if k == 1:
            remap = torch.full((1, mt), CANARY, dtype=torch.int32, device="cuda")
            tracks.retire(["a"], min_hits=3, max_age=0, tentative_age=0, remap_out=remap)
            assert np.array_equal(remap.cpu().numpy()[0], L.retire_ref(words["a"][0], words["a"][1], 3, 0, 0))
    assert tracks.enqueues == 6 and tracks.life_enqueues == 7 and int(words["a"][1][0]) == 6 and int(words["b"][1][0]) == 3
    for name in "ab":
        s = tracks._slots[name]
        assert np.array_equal(tracks._store[s].cpu().numpy(), words[name][0]) and np.array_equal(tracks._life[s].cpu().numpy(), words[name][1])
        view = tracks.life(name)
        assert int(view["step"]) == words[name][1][0] and view["uid"].data_ptr() == tracks._life[s][4:].data_ptr()
        assert np.array_equal(view["last"].cpu().numpy(), L.life_fields(words[name][1])["last"])
    # the life grows with the store
    for k in range(12):
        tracks.update(["more%d" % k], cuda(steps[0]["corners"][:1]), cuda(steps[0]["prob"][:1]), cuda(steps[0]["mask"][:1]))
    assert tracks._life.shape[0] == tracks._store.shape[0] >= 14
    assert np.array_equal(tracks._life[tracks._slots["a"]].cpu().numpy(), words["a"][1])


def _decoder_case():
    import test_gpu_scene_tracks as G
    return G._upright_outputs()


def test_only_life_to_host_synchronises():
    dec, outs, T_wl, names = _decoder_case()
    clean = [dict(o) for o in outs]                                          # track() writes into the dict it is given
    tracks = SceneTracks(max_tracks=64, num_classes=dec.num_semcls + 1, lifecycle=True)
    pose = Pose(T_wl)
    out = dec.track(outs, pose, names, tracks)                               # warm-up: allocations, library load
    corners, prob, mask = out["pred_corners_world"].clone(), out["sem_cls_prob"].clone(), out["pred_mask"].clone()
    uid, hits = torch.empty_like(out["track_id"]), torch.empty_like(out["track_id"])
    remap = torch.empty(2, 64, dtype=torch.int32, device="cuda")
    tracks.update(names, corners, prob, mask, uid_out=uid, hits_out=hits)
    tracks.retire()
    tracks.confirmed(names[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ids = tracks.update(names, corners, prob, mask, uid_out=uid, hits_out=hits)
        tracks.retire(remap_out=remap)
        tracks.retire([names[1]], min_hits=1, max_age=-1, tentative_age=-1)
        view = tracks.life(names[0])
        keep = tracks.confirmed(names[0], min_hits=3)
        out = dec.track(outs, pose, names, tracks)
        with pytest.raises(RuntimeError):
            tracks.life_to_host()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert set(out) >= {"track_id", "track_uid", "track_hits"} and out["track_uid"].dtype == torch.int32 and out["track_uid"].shape == ids.shape
    det = ids >= 0
    assert int(det.sum()) >= 6 and torch.equal(ids, out["track_id"]) and torch.equal(uid, out["track_uid"])
    assert torch.equal(uid[det], ids[det]) and bool((hits[det] == 3).all()) and bool((out["track_hits"][det] == 4).all())
    assert bool((uid[~det] == -1).all()) and bool((out["track_hits"][~det] == 0).all())
    n = int(det[0].sum())
    assert keep.dtype == torch.bool and keep.shape == (64,) and keep[:n].all() and not keep[n:].any() and int(view["step"]) == 4
    assert remap[0, :n].tolist() == list(range(n)) and bool((remap[0, n:] == -1).all())
    plain = dec.track(clean, pose, names, SceneTracks(max_tracks=64, num_classes=dec.num_semcls + 1))
    assert "track_uid" not in plain and "track_hits" not in plain and "track_id" in plain


def test_lifecycle_off_is_the_store_as_it_was():
    steps = L.scatter_steps(9, 3, 20, 3, 30)
    built = [SceneTracks(max_tracks=32), SceneTracks(max_tracks=32, lifecycle=False), SceneTracks(max_tracks=32, lifecycle=True)]
    ids = [[t.update(["x", "y", "x"], cuda(st["corners"]), cuda(st["prob"]), cuda(st["mask"])) for st in steps] for t in built]
    for other in (1, 2):
        assert all(torch.equal(a, b) for a, b in zip(ids[0], ids[other]))
        assert torch.equal(built[0]._store, built[other]._store) and built[0].enqueues == built[other].enqueues == 6
    assert built[0]._life is None and built[1]._life is None and built[0].life_enqueues == built[1].life_enqueues == 0
    assert built[2]._life is not None and built[2].life_enqueues == 6
    for call in (built[1].retire, built[1].life_to_host, lambda: built[1].life("x"), lambda: built[1].confirmed("x")):
        with pytest.raises(ValueError, match="lifecycle=True"):
            call()


def test_confirmed_is_draw_boxes_keep():
    """Six boxes in front of a camera, three of them seen three times: drawing boxes(name) with keep=confirmed(name) equals drawing
    the boxes a host-side filter of life_to_host selects."""
    H, W, Q = 48, 64, 8
    centers = [(-2.0, -1.0), (0.0, -1.0), (2.0, -1.0), (-2.0, 1.0), (0.0, 1.0), (2.0, 1.0)]
    tracks = SceneTracks(max_tracks=16, lifecycle=True)
    for k in range(3):
        corners = np.zeros((1, Q, 8, 3), np.float32)
        prob = np.zeros((1, Q, 10), np.float32)
        prob[..., 9] = 1.0
        for j, (x, y) in enumerate(centers):
            if k == 0 or j % 2 == 0:
                corners[0, j] = _yaw_box_corners(np.array([x + 0.01 * k, y, 5.0]), np.array([0.4, 0.3, 0.5]), 0.2 * j)
                prob[0, j] = 0.02
                prob[0, j, j] = 0.82
        tracks.update(["room"], cuda(corners), cuda(prob), torch.ones(1, Q, dtype=torch.bool, device="cuda"))
    rng = np.random.default_rng(5)
    images = cuda(rng.standard_normal((1, 1, 3, H, W)).astype(np.float32))
    camera = cuda(np.array([[[W, H, 20.0, 20.0, W / 2, H / 2]]], np.float32))
    pose = cuda(np.array([[[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]]], np.float32))
    view, keep = tracks.boxes("room"), tracks.confirmed("room", min_hits=3)
    got = draw_boxes(images, camera, pose, pose, view["corners"][None], view["labels"][None], keep=keep[None], count=view["count"][None],
                     num_semcls=9)
    host = [e for e in tracks.life_to_host("room") if e[5] >= 3]
    assert [e[3] for e in host] == [0, 2, 4] and keep.tolist() == [True, False, True, False, True] + [False] * 11
    want = draw_boxes(images, camera, pose, pose, cuda(np.stack([e[1] for e in host]))[None], cuda(np.array([e[0] for e in host], np.int32))[None],
                      num_semcls=9)
    base = draw_boxes(images, camera, pose, pose, view["corners"][None], view["labels"][None], keep=torch.zeros_like(keep)[None], num_semcls=9)
    everything = draw_boxes(images, camera, pose, pose, view["corners"][None], view["labels"][None], count=view["count"][None], num_semcls=9)
    assert torch.equal(got, want) and not torch.equal(got, base) and not torch.equal(got, everything)
