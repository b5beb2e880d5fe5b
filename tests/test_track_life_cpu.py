"""CPU tier of the tracks' life (parq_amd/scene_tracks.py lifecycle=True, include/parq_hip.h parq_tracks_note / parq_tracks_retire):
the NumPy statements of tests/track_life_cases.py against a second, list-of-objects formulation, their invariants after every step,
the unbounded stream that a store without retirement cannot follow, the entry points' declaration and binding, and the argument
checks that return before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import parq_amd
from parq_amd import _lib
from parq_amd.scene_tracks import SceneTracks, check_life_out, check_retire_args

import scene_tracks_cases as T
import track_life_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("parq_tracks_life_bytes", "parq_tracks_note", "parq_tracks_retire")


def sequences():
    """(name, max_tracks, conf, [per step (corners (Q,8,3), prob, mask)], steps after which a retire runs, its rule): the tracker
    case's three scenes, two more seeds of its generator on a store they overflow, and the stream."""
    out = []
    c = T.TRACKER_CASE
    for seed, mt, rule, after in ((c["seed"], c["max_tracks"], dict(min_hits=2, max_age=1, tentative_age=0), (1, 2, 3)),
                                  (11, 20, dict(min_hits=2, max_age=0, tentative_age=0), (0, 2)),
                                  (12, 96, dict(min_hits=3, max_age=-1, tentative_age=1), (2, 3))):
        steps = T.tracker_steps(dict(c, seed=seed))
        for b, name in enumerate(c["scenes"]):
            out.append(("%s/%d" % (name, seed), mt, c["conf"], [(st["corners"][b], st["prob"][b], st["mask"][b]) for st in steps], after, rule))
    out.append(("stream", L.STREAM["max_tracks"], L.STREAM["conf"], [(st["corners"][0], st["prob"][0], st["mask"][0]) for st in L.stream_steps()],
                tuple(range(len(L.stream_steps()))), L.STREAM["retire"]))
    return out


def test_statement_equals_the_list_of_objects_and_keeps_its_invariants():
    retires = drops = 0
    for name, mt, conf, steps, retire_after, rule in sequences():
        store, life = np.zeros(L.store_words(mt), np.int32), np.zeros(L.life_words(mt), np.int32)
        objects = L.LifeList()
        births, appearances = 0, {}
        for k, (corners, prob, mask) in enumerate(steps):
            what = (name, k)
            n_before = int(store[0])
            track_id, uid, hits = L.slot_step(store, life, corners, prob, mask, conf)
            want = objects.note(store, mt, track_id)
            assert [(int(u), int(h)) for u, h in zip(uid, hits)] == want, what
            objects.assert_equals(store, life, what)
            births += int(store[0]) - n_before
            for u in uid[uid >= 0].tolist():
                appearances[u] = appearances.get(u, 0) + 1
            n = int(store[0])
            F = L.life_fields(life)
            assert len(set(F["uid"][:n].tolist())) == n, what                          # the uids of a slot are distinct
            assert int(life[2]) == births and int(life[0]) == k + 1 and int(life[1]) == n, what
            assert [int(h) for h in F["hits"][:n]] == [appearances.get(int(u), 0) for u in F["uid"][:n]], what
            assert (F["first"][:n] <= F["last"][:n]).all() and (F["last"][:n] < life[0]).all() and (F["first"][:n] >= 0).all(), what
            assert ((uid == track_id) | (track_id >= 0)).all() and (hits[track_id < 0] == 0).all() and (hits[track_id >= 0] >= 1).all(), what
            if k not in retire_after:
                continue
            before_s, before_l = store.copy(), life.copy()
            remap = L.retire_ref(store, life, **rule)
            assert remap.tolist() == objects.retire(**rule) + [-1] * (mt - n), what
            objects.assert_equals(store, life, what)
            m = int(store[0])
            kept = np.nonzero(remap >= 0)[0]
            assert len(kept) == m and np.array_equal(remap[kept], np.arange(m)) and (kept < n).all(), what   # strictly increasing
            Sb, Sa = L.store_fields(before_s, mt), L.store_fields(store, mt)
            Fb, Fa = L.life_fields(before_l), L.life_fields(life)
            for key in ("labels", "scores", "corners"):                                # the kept rows are the old rows bit for bit,
                a, b = Sa[key].view(np.int32), Sb[key].view(np.int32)
                assert np.array_equal(a[:m], b[kept]) and np.array_equal(a[m:], b[m:]), (what, key)   # rows from m on are untouched
            for key in Fa:
                assert np.array_equal(Fa[key][:m], Fb[key][kept]) and np.array_equal(Fa[key][m:], Fb[key][m:]), (what, key)
            assert store[1] == before_s[1] and life[0] == before_l[0] and life[2] == before_l[2] and life[3] == before_l[3] + (n - m), what
            retires += 1
            drops += n - m
    print("retires: %d, tracks removed: %d" % (retires, drops))
    assert retires > 40 and drops > 60


def test_statement_leaves_an_invalid_slot_untouched():
    mt = 8
    for words in (dict(count=9), dict(count=-1), dict(known=5), dict(known=-1), dict(step=-1), dict(step=L.IMAX), dict(next_uid=-1),
                  dict(next_uid=L.IMAX - 1)):
        store, life = np.zeros(L.store_words(mt), np.int32), np.zeros(L.life_words(mt), np.int32)
        store[0], life[0], life[1], life[2] = 4, 3, 2, 2
        store[0] = words.get("count", store[0])
        for i, key in enumerate(("step", "known", "next_uid")):
            life[i] = words.get(key, life[i])
        before = store.copy(), life.copy()
        uid, hits = L.note_ref(store, life, np.array([0, 3, -1, -2, 77]))
        assert (uid == -1).all() and (hits == 0).all() and np.array_equal(store, before[0]) and np.array_equal(life, before[1]), words
        assert (L.retire_ref(store, life, 1, 0, 0) == -1).all() and np.array_equal(store, before[0]) and np.array_equal(life, before[1])
    # an update that has not been noted: note takes it, retire does not
    store, life = np.zeros(L.store_words(mt), np.int32), np.zeros(L.life_words(mt), np.int32)
    store[0], life[0], life[1], life[2] = 4, 3, 2, 2
    before = store.copy(), life.copy()
    assert (L.retire_ref(store, life, 1, 0, 0) == -1).all() and np.array_equal(store, before[0]) and np.array_equal(life, before[1])
    uid, hits = L.note_ref(store, life, np.array([0, 3, -1, -2, 77, 4]))
    assert uid.tolist() == [0, 3, -1, -2, -1, -1] and hits.tolist() == [1, 1, 0, 0, 0, 0] and life[:4].tolist() == [4, 4, 4, 0]
    assert L.life_fields(life)["hits"][:4].tolist() == [1, 0, 0, 1] and L.life_fields(life)["uid"][:4].tolist() == [0, 0, 2, 3]


def test_unbounded_stream_needs_retirement():
    c = L.STREAM
    steps = L.stream_steps()
    T.assert_decision_safe(steps, c["conf"])                  # first: no IoU near the threshold, re-observations clearly above it
    for st_a, st_b in zip(steps, steps[1:]):                  # a re-observation overlaps its predecessor by far more than 0.1
        for j, q in zip(st_b["objects"], st_b["queries"]):
            if j in st_a["objects"]:
                assert T.box_iou(st_b["corners"][0, q], st_a["corners"][0, st_a["queries"][st_a["objects"].index(j)]]) > 0.8
    assert len(steps) == 42 and max(len(st["objects"]) for st in steps) == 3
    plain = L.run_stream(retire=False)
    assert plain["dropped"] > 0 and any((ids == -2).any() for ids in plain["ids"]) and plain["counts"][-1] == c["max_tracks"]
    kept = L.run_stream(retire=True)
    assert kept["dropped"] == 0 and not any((ids == -2).any() for ids in kept["ids"]) and max(kept["counts"]) <= c["max_tracks"]
    assert all(len(u) == 1 for u in kept["uids"].values())                            # one uid per object, whatever its position was
    assert sorted(next(iter(u)) for u in kept["uids"].values()) == list(range(c["objects"]))
    assert int(kept["life"][3]) + int(kept["store"][0]) == c["objects"] and int(kept["life"][2]) == c["objects"]


def test_header_declares_the_entry_points_and_the_binding_types_them():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    want = {"parq_tracks_life_bytes": ["S_cap", "max_tracks"],
            "parq_tracks_note": ["store", "life", "S_cap", "max_tracks", "slots_host", "B", "track_id", "Q", "uid_out", "hits_out", "stream"],
            "parq_tracks_retire": ["store", "life", "S_cap", "max_tracks", "slots_host", "B", "min_hits", "max_age", "tentative_age",
                                   "remap_out", "stream"]}
    for name, names in want.items():
        m = re.search(r"\b(?:int|size_t)\s+\(%s\)\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/parq_hip.h must declare %s" % name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names, name
        assert name in _lib.LIFE_SYMBOLS and not any(name in t for t in _lib.ALL_TABLES + (_lib.EVAL_SYMBOLS,))
        res, args = _lib.LIFE_SYMBOLS[name]
        assert len(args) == len(names) and res is (C.c_size_t if name.endswith("bytes") else C.c_int)
    assert len(_lib.LIFE_SYMBOLS) == 3
    assert re.search(r"\b99\b", open(os.path.join(ROOT, "README.md")).read())
    assert "## Long-running streams" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert parq_amd.SceneTracks is SceneTracks


def test_library_exports_the_entry_points_and_refuses_bad_arguments_before_any_device_call():
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.LIFE_SYMBOLS[name][1] and fn.restype is _lib.LIFE_SYMBOLS[name][0]
    assert lib.parq_tracks_life_bytes(3, 96) == 3 * (4 + 4 * 96) * 4 and lib.parq_tracks_life_bytes(0, 8) == 0
    assert lib.parq_tracks_life_bytes(1, 2049) == 0 and lib.parq_tracks_life_bytes(1, 0) == 0 and lib.parq_tracks_life_bytes(-1, 8) == 0
    p = C.c_void_p(4096)                                   # non-NULL, never touched: PARQ_ERR_ARG (1) comes from checks on the host
    slots = (C.c_int32 * 2)(0, 1)

    def note(store=p, life=p, S_cap=2, mt=8, sl=slots, B=2, tid=p, Q=8):
        return lib.parq_tracks_note(store, life, S_cap, mt, sl, B, tid, Q, None, None, None)

    def retire(store=p, life=p, S_cap=2, mt=8, sl=slots, B=2, min_hits=1):
        return lib.parq_tracks_retire(store, life, S_cap, mt, sl, B, min_hits, 0, 0, None, None)
    assert note(B=0) == 0 and retire(B=0) == 0                                 # no scene: valid, nothing launched
    common = (dict(mt=0), dict(mt=2049), dict(B=-1), dict(S_cap=-1), dict(store=None), dict(life=None), dict(sl=None), dict(S_cap=1),
              dict(sl=(C.c_int32 * 2)(1, 1)), dict(sl=(C.c_int32 * 2)(0, -1)), dict(sl=(C.c_int32 * 2)(0, 2)))
    for bad in common + (dict(Q=0), dict(Q=2049), dict(tid=None)):
        assert note(**bad) == 1, bad
    assert b"parq_tracks_note" in lib.parq_last_error()
    for bad in common + (dict(min_hits=0), dict(min_hits=-3)):
        assert retire(**bad) == 1, bad
    assert b"parq_tracks_retire" in lib.parq_last_error()


def test_python_surface_checks_its_arguments_before_the_gpu():
    off = SceneTracks(max_tracks=8)
    assert off.lifecycle is False and off._life is None and SceneTracks(max_tracks=8, lifecycle=True).lifecycle is True
    z = dict(corners_world=torch.zeros(2, 5, 8, 3), sem_cls_prob=torch.zeros(2, 5, 10), pred_mask=torch.zeros(2, 5, dtype=torch.bool))
    out = torch.zeros(2, 5, dtype=torch.int32)
    for call in (lambda: off.retire(), lambda: off.retire(["a"]), lambda: off.life("a"), lambda: off.confirmed("a"),
                 lambda: off.life_to_host(), lambda: off.update(["a", "b"], uid_out=out, **z),
                 lambda: off.update(["a", "b"], hits_out=out, **z)):
        with pytest.raises(ValueError, match="lifecycle=True"):
            call()
    on = SceneTracks(max_tracks=8, lifecycle=True)
    with pytest.raises(ValueError, match="ground truth has no life"):
        on.update_labelled(["a"], torch.zeros(1, 3, 8, 3), torch.zeros(1, 3, dtype=torch.int64), torch.ones(1, 3, dtype=torch.bool))
    assert check_retire_args(["a", "b"], 3, 30, 1) == ["a", "b"] and check_retire_args([], 1, -1, -1) == []
    for names, rule, match in ((["a", "b", "a"], (3, 30, 1), "'a' is listed twice"), (["a"], (0, 30, 1), "min_hits = 0"),
                               (["a"], (-1, 30, 1), "min_hits = -1"), (["a"], (True, 30, 1), "min_hits must be"),
                               (["a"], (3, 1.5, 1), "max_age must be"), (["a"], (3, 30, None), "tentative_age must be"),
                               (["a"], (3, 2 ** 31, 1), "max_age must be")):
        with pytest.raises(ValueError, match=match):
            check_retire_args(names, *rule)
    with pytest.raises(ValueError, match="listed twice"):
        on.retire(["a", "a"])
    with pytest.raises(KeyError):
        on.retire(["nowhere"])
    on.retire()                                                               # no scene yet: nothing to do, nothing touched
    assert on.life_enqueues == 0 and on.life_to_host() == {}
    check_life_out(out, "uid_out", 2, 5)
    for bad in (torch.zeros(2, 5), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(5, 2, dtype=torch.int32).t(), None, np.zeros((2, 5), np.int32)):
        with pytest.raises(ValueError, match="uid_out must be a contiguous int32 \\(2, 5\\) tensor"):
            check_life_out(bad, "uid_out", 2, 5)
    from parq_amd.decoder import PARQDecoder
    assert "track_uid" in PARQDecoder.track.__doc__
