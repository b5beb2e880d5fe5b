"""The device tracker's rules as NumPy statements, and the seeded cases of its tests (test_scene_tracks_cpu.py,
test_gpu_scene_tracks.py).

``assign_statement`` is the assignment of include/parq_hip.h parq_assign_max: shortest augmenting paths on cost = -float64(m),
float64 duals from 0, rows in index order, on the transpose when there are more rows than columns.  THE TIE RULE is fixed here:
among unscanned columns of equal path cost an unassigned column comes before an assigned one, then the lower index.  The kernel
must reproduce this function's output exactly, ties included; every sum below is one float64 operation in the written order.

``tracks_step`` is the tracker rule of parq_tracks_update on one scene (selection, IoU, assignment, matches, births), the IoU
taken from the host routine parq_amd/f1_eval.py iou3d on ``canon`` corners and rounded to float32.
"""
import itertools
import os

import numpy as np

import golden_util as G
from oracle.make_golden import F1_CASE, _yaw_box_corners, f1_case_inputs
from parq_amd.f1_eval import F1Calculator, iou3d

FACE_ORDER = [4, 0, 1, 5, 7, 3, 2, 6]
COS_HALF_PI = 6.123233995736766e-17
assert COS_HALF_PI == float(np.cos(np.pi / 2))


# ---- part 1: the assignment ------------------------------------------------------------------------------------------------
def assign_statement(m, with_duals=False):
    """row_to_col (n_rows,) int32 of the float32 matrix m (-1: unassigned); with_duals: also (u (n_rows,), v (n_cols,)) float64,
    the duals of cost = -m in m's orientation."""
    m = np.asarray(m, np.float32)
    nr, nc = m.shape
    tr = nr > nc
    cost = -(m.T if tr else m).astype(np.float64)
    n, k = cost.shape
    u, v = np.zeros(n), np.zeros(k)
    col4row, row4col = -np.ones(n, np.int64), -np.ones(k, np.int64)
    for cur in range(n):
        sp = np.full(k, np.inf)
        path = -np.ones(k, np.int64)
        scanned = np.zeros(k, bool)
        min_val, i, sink = 0.0, cur, -1
        while sink < 0:
            open_cols = np.nonzero(~scanned)[0]
            r = ((min_val + cost[i, open_cols]) - u[i]) - v[open_cols]
            better = r < sp[open_cols]
            sp[open_cols[better]] = r[better]
            path[open_cols[better]] = i
            # least path cost; among equal ones an unassigned column first, then the lower index
            j = min(open_cols.tolist(), key=lambda c: (sp[c], row4col[c] >= 0, c))
            min_val = sp[j]
            scanned[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
        for j in np.nonzero(scanned)[0]:
            d = min_val - sp[j]
            if row4col[j] >= 0:
                u[row4col[j]] = u[row4col[j]] + d
            v[j] = v[j] - d
        u[cur] = u[cur] + min_val
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    r2c = (row4col if tr else col4row).astype(np.int32)
    if with_duals:
        return r2c, (v if tr else u), (u if tr else v)
    return r2c


def check_assignment_shape(r2c, nr, nc):
    """Every row of the smaller side used once, columns distinct and in range."""
    used = r2c[r2c >= 0]
    assert len(r2c) == nr and len(used) == min(nr, nc) and len(set(used.tolist())) == len(used)
    assert ((r2c >= -1) & (r2c < max(nc, 1))).all()


def total(m, r2c):
    return float(sum(float(m[r, c]) for r, c in enumerate(r2c.tolist()) if c >= 0))


def positive_pairs(m, r2c):
    return {(r, c) for r, c in enumerate(np.asarray(r2c).tolist()) if c >= 0 and m[r, c] > 0}


DENSE_SHAPES = [(1, 1), (1, 70), (70, 1), (5, 5), (33, 64), (64, 65), (65, 64), (130, 257), (40, 300)]


def dense_matrix(shape, seed):
    return np.random.RandomState(seed).uniform(0, 1, shape).astype(np.float32)


def iou_like_matrix(shape, seed):
    """Mostly zeros, up to three positives per row: the shape of a tracker's IoU matrix.  Ties everywhere."""
    rng = np.random.RandomState(seed)
    m = np.zeros(shape, np.float32)
    for r in range(shape[0]):
        for c in rng.choice(shape[1], size=min(shape[1], rng.randint(0, 4)), replace=False):
            m[r, c] = rng.uniform(0.02, 0.9)
    return m


def hard_matrix(n=64):
    """m[i][j] = (i+1)(j+1)/n^2: the unique optimum is the identity and every row's search runs a long augmenting path."""
    i = np.arange(1, n + 1, dtype=np.float64)
    return (np.outer(i, i) / (n * n)).astype(np.float32)


def brute_force_best(m):
    nr, nc = m.shape
    small, big = min(nr, nc), max(nr, nc)
    mm = m.T if nr > nc else m
    return max(sum(float(mm[r, c]) for r, c in enumerate(p)) for p in itertools.permutations(range(big), small))


def iou_like_cases():
    """60 IoU-like matrices of random shapes below 50 x 50, and five larger ones past one wave of columns or rows."""
    out = []
    for seed in range(60):
        rng = np.random.RandomState(1000 + seed)
        out.append(iou_like_matrix((int(rng.randint(1, 50)), int(rng.randint(1, 50))), seed))
    return out + [iou_like_matrix(s, 200 + k) for k, s in enumerate([(30, 80), (80, 30), (64, 64), (7, 130), (129, 5)])]


def small_cases():
    """A dense and an IoU-like matrix of every shape up to 6 x 6: the brute-force cases."""
    rng = np.random.RandomState(5)
    out = []
    for nr, nc in itertools.product(range(1, 7), repeat=2):
        out += [rng.uniform(0, 1, (nr, nc)).astype(np.float32), iou_like_matrix((nr, nc), 10 * nr + nc)]
    return out


def launch_matrices():
    """Every matrix of the CPU tier, plus a 0 x n, an n x 0 and an all-zero segment: the segments of the GPU tier's ONE launch."""
    mats = [dense_matrix(s, 100 + k) for k, s in enumerate(DENSE_SHAPES)] + iou_like_cases() + [hard_matrix(64)] + small_cases()
    return mats + [np.zeros((0, 9), np.float32), np.zeros((9, 0), np.float32), np.zeros((6, 6), np.float32)]


# ---- part 2: the tracker -----------------------------------------------------------------------------------------------------
def canon(corners_f32):
    """canonical() as parq_tracks_update computes it: float64 from the float32 corners, re-ordered, (x, c y - z, y + c z)."""
    w = np.asarray(corners_f32, np.float32).astype(np.float64)[FACE_ORDER]
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    return np.stack([x, COS_HALF_PI * y - z, y + COS_HALF_PI * z], axis=1)


_IOU_MEMO = {}


def box_iou(a_f32, b_f32):
    """float64 host IoU of two float32 world boxes (memoised: the set-up re-runs trackers on the same pairs); 0 for a box with
    a non-finite corner."""
    a, b = np.ascontiguousarray(a_f32, np.float32), np.ascontiguousarray(b_f32, np.float32)
    key = (a.tobytes(), b.tobytes())
    if key not in _IOU_MEMO:
        ok = np.isfinite(a).all() and np.isfinite(b).all()
        _IOU_MEMO[key] = float(iou3d(canon(a), canon(b))[0]) if ok else 0.0
    return _IOU_MEMO[key]


def empty_store(max_tracks):
    return dict(count=0, dropped=0, labels=np.zeros(max_tracks, np.int32), scores=np.zeros(max_tracks, np.float32),
                corners=np.zeros((max_tracks, 8, 3), np.float32))


def select(prob, mask, conf):
    """(detection queries in order, labels, float32 scores) of one scene."""
    prob = np.asarray(prob, np.float32)
    K = prob.shape[1]
    qs, labels, scores = [], [], []
    for q in range(prob.shape[0]):
        row = prob[q]
        if np.isnan(row).any():
            continue
        arg = int(np.argmax(row))
        if arg != K - 1 and row[arg] > np.float32(conf) and mask[q]:
            qs.append(q)
            labels.append(arg)
            scores.append(row[arg])
    return qs, labels, scores


def tracks_step(store, corners, prob, mask, conf, iou_thresh, iou_scale=None):
    """One scene, one step, in place on `store`; returns (track_id (Q,) int32, IoU (D, n) float32, info).  iou_scale: a function
    (D, n) float64 -> factors, for the decision-safety runs."""
    mt = len(store["labels"])
    Q = prob.shape[0]
    n = store["count"]
    track_id = -np.ones(Q, np.int32)
    qs, labels, scores = select(prob, mask, conf)
    D = len(qs)
    iou64 = np.array([[box_iou(corners[q], store["corners"][t]) for t in range(n)] for q in qs], np.float64).reshape(D, n)
    if iou_scale is not None:
        iou64 = iou64 * iou_scale(iou64)
    iou = iou64.astype(np.float32)
    r2c = assign_statement(iou) if n > 0 else -np.ones(D, np.int32)
    births = replaced = 0
    for d, q in enumerate(qs):
        c = int(r2c[d])
        if c >= 0 and not (iou[d, c] < np.float32(iou_thresh)):
            track_id[q] = c
            if store["scores"][c] < scores[d]:
                store["labels"][c], store["scores"][c], store["corners"][c] = labels[d], scores[d], corners[q]
                replaced += 1
            continue
        pos = n + births
        births += 1
        if pos < mt:
            store["labels"][pos], store["scores"][pos], store["corners"][pos] = labels[d], scores[d], corners[q]
            track_id[q] = pos
        else:
            track_id[q] = -2
            store["dropped"] += 1
    store["count"] = min(n + births, mt)
    return track_id, iou, dict(D=D, n=n, births=births, replaced=replaced, iou64=iou64)


def run_statement(steps, max_tracks, conf, iou_thresh=0.1, iou_scale=None):
    """All steps on fresh stores: ({name: store}, per step {"track_id" (B,Q), "ious" [per scene], "info" [per scene],
    "stores" deep copy after the step})."""
    stores, trace = {}, []
    for st in steps:
        ids, ious, infos = [], [], []
        for b, name in enumerate(st["scenes"]):
            store = stores.setdefault(name, empty_store(max_tracks))
            tid, iou, info = tracks_step(store, st["corners"][b], st["prob"][b], st["mask"][b], conf, iou_thresh, iou_scale)
            ids.append(tid)
            ious.append(iou)
            infos.append(info)
        trace.append(dict(track_id=np.stack(ids), ious=ious, info=infos,
                          stores={n: {k: (v.copy() if hasattr(v, "copy") else v) for k, v in s.items()} for n, s in stores.items()}))
    return stores, trace


def store_tracks(store):
    """Sorted [(class, score, corner bytes)] of a statement store."""
    return sorted((int(store["labels"][t]), float(store["scores"][t]), store["corners"][t].tobytes()) for t in range(store["count"]))


def entry_tracks(entries):
    """Sorted [(class, score, corner bytes)] of F1Calculator entries."""
    return sorted((int(e[0]), float(e[2]), np.ascontiguousarray(e[1], np.float32).tobytes()) for e in entries)


def host_run(steps, conf, iou_backend=None, seed=99):
    """The unmodified host tracker on the steps (ground truth included when the steps carry it)."""
    import torch
    calc = F1Calculator(conf, iou_backend=iou_backend)
    np.random.seed(seed)
    for st in steps:
        out = {"pred_corners_world": torch.from_numpy(st["corners"]), "sem_cls_prob": torch.from_numpy(st["prob"]),
               "pred_mask": torch.from_numpy(st["mask"]), "scene_name": st["scenes"]}
        gts = st.get("gts") or [dict(labels=np.zeros(0, np.int64), corners=np.zeros((0, 8, 3), np.float32)) for _ in st["scenes"]]
        calc.step(out, [{"labels": torch.from_numpy(x["labels"]), "gt_corners_world": torch.from_numpy(x["corners"])} for x in gts])
    return calc


class ScaledBackend:
    """host_iou_backend with the positive IoUs scaled by 1 + 1e-7 * N(0, 1): a tracker whose decisions survive this does not
    hang on the last bits of an IoU."""

    def __init__(self, noise_seed):
        self.rng = np.random.RandomState(noise_seed)

    def __call__(self, segments):
        out = []
        for m in memo_iou_backend(segments):
            out.append(m * (1.0 + 1e-7 * self.rng.standard_normal(m.shape)))
        return out


def memo_iou_backend(segments):
    """host_iou_backend, memoised per pair of canonical boxes."""
    out = []
    for A, B in segments:
        m = np.zeros((len(A), len(B)), np.float64)
        for i, a in enumerate(A):
            for j, b in enumerate(B):
                key = (a.tobytes(), b.tobytes(), "c")
                if key not in _IOU_MEMO:
                    _IOU_MEMO[key] = float(iou3d(a, b)[0])
                m[i, j] = _IOU_MEMO[key]
        out.append(m)
    return out


def assert_decision_safe(steps, conf, iou_thresh=0.1):
    """The generators' promise: no float64 IoU within 1e-6 of the threshold, and the host tracker, re-run with every positive IoU
    scaled by 1 + 1e-7 * noise for three noise seeds, ends in the same state."""
    def tracker_state(calc):                                          # bytes, not values: a NaN corner must compare equal to itself
        return [{n: [(int(e[0]), float(e[2]), np.ascontiguousarray(e[1], np.float32).tobytes(), int(e[3])) for e in trks]
                 for n, trks in calc.preds.items()}]
    seen = []

    def recording(segments):
        mats = memo_iou_backend(segments)
        seen.extend(mats)
        return mats
    base = tracker_state(host_run(steps, conf, iou_backend=recording))[0]
    allv = np.concatenate([m.reshape(-1) for m in seen]) if seen else np.zeros(0)
    assert not (np.abs(allv - iou_thresh) < 1e-6).any()
    for noise_seed in (1, 2, 3):
        assert tracker_state(host_run(steps, conf, iou_backend=ScaledBackend(noise_seed)))[0] == base, noise_seed
    return base


def g12_steps():
    return f1_case_inputs(F1_CASE)


def g12_golden():
    return np.load(os.path.join(G.GOLDEN_DIR, "g12_f1.npz"))


TRACKER_CASE = dict(seed=4107, scenes=["s0", "s1", "s2"], Q=70, K=10, max_tracks=96, steps=4, nbox=12, conf=0.1, iou=0.1)


def _detection_row(rng, cls, boost):
    logits = rng.normal(0, 1, 10)
    logits[cls] += boost
    e = np.exp(logits - logits.max())
    return (e / e.sum()).astype(np.float32)


def tracker_steps(c=TRACKER_CASE):
    """Four steps of three scenes, Q = 70 (past one wave).  Together they hold a first visit, D < n, D > n (scene s1 sees two
    detections first and many afterwards), D = 0 (s2 in step 2 is masked out), a replacement by a more confident detection (s0,
    step 1, query 30 repeats step 0's first detection with probability 0.995), a NaN-probability row and two boxes with a
    non-finite corner (NaN, inf).  Asserted in the set-up (`tracker_case`)."""
    rng = np.random.RandomState(c["seed"])
    S, Q, nb = len(c["scenes"]), c["Q"], c["nbox"]
    world = [[dict(center=rng.uniform(-3, 3, 3) * np.array([1, 1, 0.3]), half=rng.uniform(0.25, 0.6, 3), yaw=rng.uniform(-np.pi, np.pi),
                   cls=int(rng.randint(0, 9))) for _ in range(nb)] for _ in range(S)]
    steps = []
    for t in range(c["steps"]):
        corners = np.zeros((S, Q, 8, 3), np.float32)
        prob = np.zeros((S, Q, c["K"]), np.float32)
        mask = np.zeros((S, Q), bool)
        for s in range(S):
            for q in range(Q):
                if q < 2 * nb and rng.rand() < 0.7:
                    bx = world[s][q % nb]
                    corners[s, q] = _yaw_box_corners(bx["center"] + rng.normal(0, 0.08, 3), bx["half"] * rng.uniform(0.8, 1.2, 3),
                                                     bx["yaw"] + rng.normal(0, 0.1))
                    prob[s, q] = _detection_row(rng, bx["cls"], rng.uniform(2.0, 4.0))
                else:
                    corners[s, q] = _yaw_box_corners(rng.uniform(-4, 4, 3) * np.array([1, 1, 0.3]), rng.uniform(0.2, 0.5, 3),
                                                     rng.uniform(-np.pi, np.pi))
                    prob[s, q] = _detection_row(rng, 9, rng.uniform(1.5, 4.0))
                mask[s, q] = rng.rand() < 0.85
        if t == 0:                                                  # s1 starts with two detections: D > n on its next visit
            keep = select(prob[1], mask[1], c["conf"])[0][:2]
            mask[1] = False
            mask[1, keep] = True
        if t == 1:
            q0 = select(steps[0]["prob"][0], steps[0]["mask"][0], c["conf"])[0][0]
            corners[0, 30] = steps[0]["corners"][0, q0] + np.float32(0.01)
            prob[0, 30] = 0.0005
            prob[0, 30, int(np.argmax(steps[0]["prob"][0, q0]))] = 0.9955
            mask[0, 30] = True
            prob[2, 5, 3] = np.nan                                  # a NaN-probability row: no detection
            mask[2, 5] = True
        if t == 2:
            mask[2] = False                                         # D = 0
        if t == 3:
            for s, q, bad in ((0, 7, np.nan), (1, 3, np.inf)):      # boxes with a non-finite corner: IoU 0 with everything, born
                corners[s, q, 2, 1] = bad
                prob[s, q] = 0.01
                prob[s, q, 2] = 0.91
                mask[s, q] = True
        steps.append(dict(scenes=list(c["scenes"]), corners=corners, prob=prob, mask=mask))
    return steps


_CASE_MEMO = {}


def tracker_case(c=TRACKER_CASE):
    """(steps, statement trace, final statement stores) of the GPU tier's tracker case, its promises asserted once."""
    if "case" not in _CASE_MEMO:
        steps = tracker_steps(c)
        stores, trace = run_statement(steps, c["max_tracks"], c["conf"], c["iou"])
        infos = [i for tr in trace for i in tr["info"]]
        assert any(i["n"] == 0 and i["D"] > 0 for i in infos) and any(0 < i["D"] < i["n"] for i in infos)
        assert any(i["D"] > i["n"] > 0 for i in infos) and any(i["D"] == 0 and i["n"] > 0 for i in infos)
        assert trace[1]["info"][0]["replaced"] >= 1 and trace[1]["track_id"][0, 30] >= 0
        assert trace[1]["track_id"][2, 5] == -1
        assert trace[3]["track_id"][0, 7] >= trace[2]["stores"]["s0"]["count"] and trace[3]["track_id"][1, 3] >= trace[2]["stores"]["s1"]["count"]
        assert all(0 < s["count"] < c["max_tracks"] and s["dropped"] == 0 for s in stores.values())
        assert sum((i["iou64"] >= 0.1).sum() for i in infos) > 40
        _CASE_MEMO["case"] = (steps, trace, stores)
    return _CASE_MEMO["case"]


def overflow_step(Q=70, births=12):
    """One scene whose first visit holds `births` far-apart detections."""
    rng = np.random.RandomState(31)
    corners = np.zeros((1, Q, 8, 3), np.float32)
    prob = np.zeros((1, Q, 10), np.float32)
    prob[..., 9] = 1.0
    mask = np.ones((1, Q), bool)
    for k, q in enumerate(sorted(rng.choice(Q, births, replace=False).tolist())):
        corners[0, q] = _yaw_box_corners(np.array([3.0 * k, 0.0, 0.0]), np.array([0.4, 0.3, 0.5]), 0.3 * k)
        prob[0, q] = 0.02
        prob[0, q, k % 9] = 0.82
    return dict(scenes=["full"], corners=corners, prob=prob, mask=mask)
