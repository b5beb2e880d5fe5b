"""The rules of the tracks' life as NumPy statements, and the seeded cases of their tests (test_track_life_cpu.py,
test_gpu_track_life.py).

``note_ref`` and ``retire_ref`` are include/parq_hip.h parq_tracks_note / parq_tracks_retire on ONE scene slot.  They work, in
place, on the same int32 word arrays as the kernels: a store slot of 2 + 26 * max_tracks words (count, dropped, labels, score bits,
corner bits) and a life slot of 4 + 4 * max_tracks words (step, known, next_uid, retired, uid, hits, first, last), and return what
the launch writes beside them.  ``slot_step`` is one update of a slot: scene_tracks_cases.tracks_step on views of the words, then
``note_ref``.  ``LifeList`` is the second formulation: a Python list of objects, appended to at a birth, deleted from at a retire.
"""
import numpy as np

from oracle.make_golden import _yaw_box_corners
from scene_tracks_cases import assert_decision_safe, empty_store, overflow_step, tracker_steps, tracks_step  # noqa: F401

IMAX = 2 ** 31 - 1


# ---- the words ---------------------------------------------------------------------------------------------------------------
def store_words(mt):
    return 2 + 26 * mt


def life_words(mt):
    return 4 + 4 * mt


def life_mt(life_slot):
    assert (len(life_slot) - 4) % 4 == 0
    return (len(life_slot) - 4) // 4


def store_fields(store_slot, mt):
    """Views of a store slot's words: labels (mt) int32, scores (mt) float32, corners (mt,8,3) float32."""
    assert store_slot.dtype == np.int32 and len(store_slot) == store_words(mt)
    return dict(labels=store_slot[2:2 + mt], scores=store_slot[2 + mt:2 + 2 * mt].view(np.float32),
                corners=store_slot[2 + 2 * mt:].view(np.float32).reshape(mt, 8, 3))


def life_fields(life_slot):
    """Views of a life slot's words: uid, hits, first, last (mt) int32."""
    mt = life_mt(life_slot)
    assert life_slot.dtype == np.int32
    return {k: life_slot[4 + f * mt:4 + (f + 1) * mt] for f, k in enumerate(("uid", "hits", "first", "last"))}


def life_valid(n, k, t0, nu, mt):
    return 0 <= n <= mt and 0 <= k <= n and 0 <= t0 < IMAX and nu >= 0 and nu + (n - k) <= IMAX


# ---- the statements ------------------------------------------------------------------------------------------------------------
def note_ref(store_slot, life_slot, track_id_row):
    """parq_tracks_note on one slot, in place on `life_slot`; returns (uid_out (Q,), hits_out (Q,)) int32."""
    mt = life_mt(life_slot)
    ids = np.asarray(track_id_row, np.int64)
    uid_out, hits_out = np.full(len(ids), -1, np.int32), np.zeros(len(ids), np.int32)
    n, t0, k, nu = int(store_slot[0]), int(life_slot[0]), int(life_slot[1]), int(life_slot[2])
    if not life_valid(n, k, t0, nu, mt):
        return uid_out, hits_out
    L = life_fields(life_slot)
    seen = np.zeros(n, bool)
    seen[ids[(ids >= 0) & (ids < n)]] = True
    for t in range(k):
        if seen[t]:
            L["hits"][t] = min(int(L["hits"][t]) + 1, IMAX)
            L["last"][t] = t0
    for t in range(k, n):
        L["uid"][t] = nu + (t - k)
        L["hits"][t] = 1 if seen[t] else 0
        L["first"][t] = L["last"][t] = t0
    life_slot[2] = nu + (n - k)
    life_slot[1] = n
    life_slot[0] = t0 + 1
    for q, i in enumerate(ids.tolist()):
        if 0 <= i < n:
            uid_out[q], hits_out[q] = L["uid"][i], L["hits"][i]
        elif i in (-1, -2):
            uid_out[q] = i
    return uid_out, hits_out


def retire_ref(store_slot, life_slot, min_hits, max_age, tentative_age):
    """parq_tracks_retire on one slot, in place on both; returns remap (max_tracks,) int32."""
    assert min_hits >= 1
    mt = life_mt(life_slot)
    remap = np.full(mt, -1, np.int32)
    n, t0, k, nu = int(store_slot[0]), int(life_slot[0]), int(life_slot[1]), int(life_slot[2])
    if not life_valid(n, k, t0, nu, mt) or k != n:
        return remap
    S, L = store_fields(store_slot, mt), life_fields(life_slot)
    scores, corners = S["scores"].view(np.int32), S["corners"].view(np.int32)
    m = 0
    for t in range(n):
        age = (t0 - 1) - int(L["last"][t])
        if int(L["hits"][t]) >= min_hits:
            drop = max_age >= 0 and age > max_age
        else:
            drop = tentative_age >= 0 and age > tentative_age
        if drop:
            continue
        if m != t:                                              # m <= t: rows are read before anything lands on them
            S["labels"][m], scores[m], corners[m] = S["labels"][t], scores[t], corners[t]
            for f in L.values():
                f[m] = f[t]
        remap[t] = m
        m += 1
    store_slot[0] = m
    life_slot[1] = m
    life_slot[3] = min(int(life_slot[3]) + (n - m), IMAX)
    return remap


def slot_step(store_slot, life_slot, corners, prob, mask, conf, iou_thresh=0.1):
    """One update of one slot's words: the tracker's statement, then note_ref.  Returns (track_id, uid_out, hits_out)."""
    mt = life_mt(life_slot)
    view = store_fields(store_slot, mt)
    view.update(count=int(store_slot[0]), dropped=int(store_slot[1]))
    track_id, _, _ = tracks_step(view, corners, prob, mask, conf, iou_thresh)
    store_slot[0], store_slot[1] = view["count"], view["dropped"]
    uid, hits = note_ref(store_slot, life_slot, track_id)
    return track_id, uid, hits


# ---- the second formulation ------------------------------------------------------------------------------------------------------
class LifeList:
    """The same rules on a Python list of objects: a birth appends, a retire deletes."""

    def __init__(self):
        self.objs, self.step, self.next_uid, self.retired = [], 0, 0, 0

    def note(self, store_slot, mt, track_id_row):
        n = int(store_slot[0])
        ids = {int(i) for i in track_id_row if 0 <= i < n}
        for t, o in enumerate(self.objs):
            if t in ids:
                o["hits"] += 1
                o["last"] = self.step
        while len(self.objs) < n:
            self.objs.append(dict(uid=self.next_uid, hits=int(len(self.objs) in ids), first=self.step, last=self.step))
            self.next_uid += 1
        S = store_fields(store_slot, mt)
        for t, o in enumerate(self.objs):                       # what the store holds for the object now (a match may replace it)
            o["label"], o["score"], o["corners"] = int(S["labels"][t]), S["scores"][t].tobytes(), S["corners"][t].tobytes()
        self.step += 1
        out = []
        for i in (int(i) for i in track_id_row):
            out.append((self.objs[i]["uid"], self.objs[i]["hits"]) if 0 <= i < n else (i if i in (-1, -2) else -1, 0))
        return out

    def retire(self, min_hits, max_age, tentative_age):
        def gone(o):
            age = (self.step - 1) - o["last"]
            limit = max_age if o["hits"] >= min_hits else tentative_age
            return limit >= 0 and age > limit
        kept = [o for o in self.objs if not gone(o)]
        remap, pos = [], 0
        for o in self.objs:
            remap.append(-1 if gone(o) else pos)
            pos += not gone(o)
        self.retired += len(self.objs) - len(kept)
        self.objs = kept
        return remap

    def assert_equals(self, store_slot, life_slot, what):
        mt = life_mt(life_slot)
        S, L = store_fields(store_slot, mt), life_fields(life_slot)
        assert (int(store_slot[0]), int(life_slot[1])) == (len(self.objs), len(self.objs)), what
        assert (int(life_slot[0]), int(life_slot[2]), int(life_slot[3])) == (self.step, self.next_uid, self.retired), what
        for t, o in enumerate(self.objs):
            got = dict(uid=int(L["uid"][t]), hits=int(L["hits"][t]), first=int(L["first"][t]), last=int(L["last"][t]),
                       label=int(S["labels"][t]), score=S["scores"][t].tobytes(), corners=S["corners"][t].tobytes())
            for key, v in o.items():
                assert got[key] == v, (what, t, key)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
STREAM = dict(objects=40, span=3, Q=6, max_tracks=8, conf=0.1, retire=dict(min_hits=2, max_age=2, tentative_age=1))


def stream_steps(c=STREAM):
    """One scene: `objects` well separated boxes (3 m apart along x), object j observed in steps j .. j + span - 1, moved by 2 cm per
    step, and never again.  Up to `span` detections per step, on changing queries."""
    steps = []
    for s in range(c["objects"] + c["span"] - 1):
        corners = np.zeros((1, c["Q"], 8, 3), np.float32)
        prob = np.zeros((1, c["Q"], 10), np.float32)
        prob[..., 9] = 1.0
        mask = np.ones((1, c["Q"]), bool)
        active = [j for j in range(c["objects"]) if j <= s < j + c["span"]]
        for i, j in enumerate(active):
            q = 2 * i + s % 2
            corners[0, q] = _yaw_box_corners(np.array([3.0 * j + 0.02 * (s - j), 0.0, 0.0]), np.array([0.4, 0.3, 0.5]), 0.3 * j)
            prob[0, q] = 0.02
            prob[0, q, j % 9] = 0.82
        steps.append(dict(scenes=["stream"], corners=corners, prob=prob, mask=mask, objects=active, queries=[2 * i + s % 2 for i in range(len(active))]))
    return steps


def run_stream(retire, c=STREAM):
    """The stream through the statement; returns dict(ids [per step], uids {object: set}, counts [after each step's update],
    dropped, store, life)."""
    mt = c["max_tracks"]
    store, life = np.zeros(store_words(mt), np.int32), np.zeros(life_words(mt), np.int32)
    ids, uids, counts = [], {}, []
    for st in stream_steps(c):
        tid, uid, _ = slot_step(store, life, st["corners"][0], st["prob"][0], st["mask"][0], c["conf"])
        ids.append(tid)
        counts.append(int(store[0]))
        for j, q in zip(st["objects"], st["queries"]):
            uids.setdefault(j, set()).add(int(uid[q]))
        if retire:
            retire_ref(store, life, **c["retire"])
    return dict(ids=ids, uids=uids, counts=counts, dropped=int(store[1]), store=store, life=life)


def scatter_steps(seed, B, Q, steps, world, p_det=0.6):
    """`steps` batches of B scenes, Q queries: every query is, with probability p_det, a noisy view (1 cm) of one of `world` boxes
    on a 3 m grid, each box at most once per scene and step, else background.  For the GPU tier, which takes track_id from the
    real update: no host IoU is ever computed on these."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(steps):
        corners = np.zeros((B, Q, 8, 3), np.float32)
        prob = np.zeros((B, Q, 10), np.float32)
        prob[..., 9] = 1.0
        mask = np.ones((B, Q), bool)
        objects = -np.ones((B, Q), np.int64)                      # the world box each query shows (-1: background)
        for b in range(B):
            picks = rng.permutation(world)[:Q]
            for q, j in enumerate(picks.tolist()):
                if rng.rand() < p_det:
                    center = np.array([3.0 * (j % 48), 3.0 * (j // 48), 0.0]) + rng.normal(0, 0.01, 3)
                    corners[b, q] = _yaw_box_corners(center, np.array([0.4, 0.3, 0.5]), 0.1 * (j % 7))
                    prob[b, q] = 0.02
                    prob[b, q, j % 9] = rng.uniform(0.5, 0.8)
                    objects[b, q] = j
        out.append(dict(corners=corners, prob=prob, mask=mask, objects=objects))
    return out


RETIRE_RULE = dict(min_hits=2, max_age=3, tentative_age=1)
DROP_PATTERNS = ("none", "all", "first", "last", "every_second", "one_chunk", "all_but_one_per_chunk", "last_chunk", "empty")


def drop_mask(pattern, n):
    t = np.arange(n)
    if pattern in ("none", "empty"):
        return np.zeros(n, bool)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "first":
        return t == 0
    if pattern == "last":
        return t == n - 1
    if pattern == "every_second":
        return t % 2 == 1
    if pattern == "one_chunk":                                   # the second whole chunk of 64 where there is one, else the first
        c0 = 64 if n >= 128 else 0
        return (t >= c0) & (t < c0 + 64)
    if pattern == "all_but_one_per_chunk":
        return t % 64 != (t // 64 * 7 + 5) % 64
    if pattern == "last_chunk":                                  # the partial last chunk only (the whole of a store below one chunk)
        return t >= (n - 1) // 64 * 64 if n % 64 else t >= n - 64
    raise ValueError(pattern)


def retire_case(mt, pattern, seed):
    """(store slot, life slot, drop mask) for RETIRE_RULE: random words everywhere, rows from the count on included, and a life
    whose hits / last make exactly the tracks of `pattern` go: confirmed and tentative tracks on both sides of their limits."""
    rng = np.random.RandomState(seed)
    n = 0 if pattern == "empty" else (mt if pattern in ("one_chunk", "last_chunk") or mt < 3 else mt - rng.randint(0, 2))
    store = rng.randint(-2 ** 31, 2 ** 31, store_words(mt), dtype=np.int64).astype(np.int32)
    life = rng.randint(-2 ** 31, 2 ** 31, life_words(mt), dtype=np.int64).astype(np.int32)
    step = 50
    store[0], store[1] = n, 7
    life[:4] = (step, n, 1000, 3)
    L = life_fields(life)
    drop = drop_mask(pattern, n)
    for t in range(n):
        confirmed = rng.rand() < 0.5
        L["hits"][t] = rng.randint(2, 9) if confirmed else rng.randint(0, 2)
        limit = RETIRE_RULE["max_age"] if confirmed else RETIRE_RULE["tentative_age"]
        age = limit + 1 + rng.randint(0, 3) if drop[t] else rng.randint(0, limit + 1)
        L["last"][t] = (step - 1) - age
        L["first"][t] = L["last"][t] - rng.randint(0, 5)
    L["uid"][:n] = rng.permutation(1000)[:n] if n <= 1000 else np.arange(n)
    return store, life, drop
