"""The rules of the evaluator's device path as NumPy statements (include/parq_hip.h parq_gt_tracks_update, parq_f1_counts), and the
seeded cases of its tests (test_f1_device_cpu.py, test_gpu_f1_device.py).

``gt_jitter`` is the hashed jitter, built from the matcher's hash (tests/set_match_cases.py mix32); ``gt_tracks_step`` is step 1 of
parq_gt_tracks_update (valid rows, jittered corners, score 1) followed by the tracker statement of tests/scene_tracks_cases.py,
unchanged; ``counts_statement`` is parq_f1_counts: best[i] per ground-truth track from ``pair_iou_statement`` (csrc/obb_pair.hpp
operation by operation, so that best_iou can be compared bit for bit), then the per-class counts.  The kernels must
reproduce these exactly.
"""
import numpy as np

import eval_iou_cases as E
import scene_tracks_cases as T
from oracle.make_golden import F1_CASE, _yaw_box_corners
from parq_amd.f1_eval import F1Calculator
from set_match_cases import GOLDEN, mix32

JITTER_UNIT = 1.7320508075688772e-3 / 65536            # the float64 2.6428997918226275e-08
assert JITTER_UNIT == 2.6428997918226275e-08
THRESHOLDS = (0.25, 0.5, 0.7)
K_CARE = 9


# ---- the jitter ---------------------------------------------------------------------------------------------------------------
def gt_jitter(seed, slot, visit, positions):
    """float64 jitter of the boxes at `positions` (array) of visit `visit` of the scene in slot `slot`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    pos = np.asarray(positions, np.uint32)
    with np.errstate(over="ignore"):
        h = np.full(len(pos), GOLDEN, np.uint32)
        for w in (seed & 0xFFFFFFFF, seed >> 32, slot, visit):
            h = mix32((h ^ np.uint32(w)) + np.uint32(GOLDEN))
        h = mix32((h ^ pos) + np.uint32(GOLDEN))
        words = [mix32((h ^ np.uint32(k)) + np.uint32(GOLDEN)) for k in (0, 1)]
    fields = [f.astype(np.int64) for w in words for f in (w & np.uint32(0xFFFF), w >> np.uint32(16))]
    u = fields[0] + fields[1] + fields[2] + fields[3] - 131070
    return u.astype(np.float64) * JITTER_UNIT


def jittered(corners_f32, jitter):
    return (np.asarray(corners_f32, np.float32).astype(np.float64) + jitter[:, None, None]).astype(np.float32)


# ---- the ground-truth store -----------------------------------------------------------------------------------------------------
def gt_tracks_step(store, corners, labels, valid, seed, slot, visit, iou_thresh=0.1):
    """One scene, one ground-truth update, in place on `store` (scene_tracks_cases.empty_store): the valid rows in row order, row of
    rank p moved by gt_jitter(seed, slot, visit, p), label labels[row], score 1, then T.tracks_step's rule.  Labels must be >= 0
    here (the tracker statement selects through a one-hot probability row).  Returns (IoU (D, n) float32, info)."""
    corners, labels, valid = np.asarray(corners, np.float32), np.asarray(labels, np.int64), np.asarray(valid).astype(bool)
    P = len(labels)
    rows = np.nonzero(valid)[0]
    moved = corners.copy()
    moved[rows] = jittered(corners[rows], gt_jitter(seed, slot, visit, np.arange(len(rows))))
    assert (labels[rows] >= 0).all()
    prob = np.zeros((P, int(labels[rows].max(initial=0)) + 2), np.float32)
    prob[rows, labels[rows]] = 1.0
    _, iou, info = T.tracks_step(store, moved, prob, valid, 0.5, iou_thresh)
    return iou, info


def gt_run_statement(steps, max_tracks, seed=0, iou_thresh=0.1, slots=None):
    """All ground-truth updates of `steps` on fresh stores: ({name: store}, per step {"stores" deep copy after the step, "ious",
    "info"}, {name: slot}).  A step is dict(scenes, gt_labels (B,P), gt_corners (B,P,8,3), gt_valid (B,P)); slots in order of first
    appearance (or as given in `slots`), a scene's visits counted per update."""
    stores, slots, visits, trace = {}, dict(slots or {}), {}, []
    for st in steps:
        ious, infos = [], []
        for b, name in enumerate(st["scenes"]):
            slot = slots.setdefault(name, len(slots))
            store = stores.setdefault(name, T.empty_store(max_tracks))
            iou, info = gt_tracks_step(store, st["gt_corners"][b], st["gt_labels"][b], st["gt_valid"][b], seed, slot, visits.get(name, 0),
                                       iou_thresh)
            visits[name] = visits.get(name, 0) + 1
            ious.append(iou)
            infos.append(info)
        trace.append(dict(ious=ious, info=infos,
                          stores={n: {k: (v.copy() if hasattr(v, "copy") else v) for k, v in s.items()} for n, s in stores.items()}))
    return stores, trace, slots


def padded(gts, P=None):
    """A list of per-scene dict(labels, corners) as dict(gt_labels (B,P) int32, gt_corners (B,P,8,3) float32, gt_valid (B,P) bool)."""
    ns = [len(g["labels"]) for g in gts]
    P = P or max(ns + [1])
    out = dict(gt_labels=np.zeros((len(gts), P), np.int32), gt_corners=np.zeros((len(gts), P, 8, 3), np.float32),
               gt_valid=np.zeros((len(gts), P), bool))
    for b, (g, n) in enumerate(zip(gts, ns)):
        out["gt_labels"][b, :n], out["gt_corners"][b, :n], out["gt_valid"][b, :n] = g["labels"], g["corners"], True
    return out


def with_padded_gt(steps):
    """The evaluator steps (eval_iou_cases) with their ground truth also in the padded form gt_run_statement reads."""
    return [dict(st, **padded(st["gts"])) for st in steps]


def label_corner_multiset(labels, corners):
    return sorted((int(l), np.ascontiguousarray(c, np.float32).tobytes()) for l, c in zip(labels, corners))


def store_multiset(store):
    return label_corner_multiset(store["labels"][:store["count"]], store["corners"][:store["count"]])


def entries_multiset(entries):
    return label_corner_multiset([e[0] for e in entries], [e[1] for e in entries])


def hash_calculator(seed=0, **kw):
    return F1Calculator(F1_CASE["conf"], gt_jitter="hash", gt_seed=seed, **kw)


# ---- the counts -------------------------------------------------------------------------------------------------------------------
def pair_iou_statement(c1, c2):
    """The 3-D IoU of two canon() boxes as csrc/obb_pair.hpp computes it: the host routine iou3d with every float64 operation
    written out in the kernel's order (the host sums its shoelace and edge lengths through NumPy reductions, whose order is
    NumPy's own; the two agree within 1e-12, test_f1_device_cpu.py).  np.float64 scalars: one rounding per operation, 1 / 0 = inf."""
    f = np.float64
    c1, c2 = [[f(v) for v in row] for row in c1], [[f(v) for v in row] for row in c2]

    def quad_area(c):
        x0, y0, x1, y1, x2, y2, x3, y3 = c[3][0], c[3][2], c[2][0], c[2][2], c[1][0], c[1][2], c[0][0], c[0][2]
        s1 = ((x0 * y3 + x1 * y0) + x2 * y1) + x3 * y2
        s2 = ((y0 * x3 + y1 * x0) + y2 * x1) + y3 * x2
        return f(0.5) * abs(s1 - s2)

    def edge(c, i, j):
        dx, dy, dz = c[i][0] - c[j][0], c[i][1] - c[j][1], c[i][2] - c[j][2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz)

    max_v = 12
    poly = [(c1[3 - k][0], c1[3 - k][2]) for k in range(4)]
    a1, a2 = quad_area(c1), quad_area(c2)
    with np.errstate(all="ignore"):
        for e in range(4):
            ka, kb = 3 - ((e + 3) & 3), 3 - e
            ax, ay, bx, by = c2[ka][0], c2[ka][2], c2[kb][0], c2[kb][2]
            ex, ey = bx - ax, by - ay
            out, m = [], 0
            qx, qy = poly[-1]
            q_in = ex * (qy - ay) > ey * (qx - ax)
            for cx, cy in poly:
                c_in = ex * (cy - ay) > ey * (cx - ax)
                if c_in != q_in:
                    dcx, dcy, dpx, dpy = ax - bx, ay - by, qx - cx, qy - cy
                    n1, n2 = ax * by - ay * bx, qx * cy - qy * cx
                    inv = f(1.0) / (dcx * dpy - dcy * dpx)
                    if m < max_v:
                        out.append(((n1 * dpx - n2 * dcx) * inv, (n1 * dpy - n2 * dcy) * inv))
                    m += 1
                if c_in:
                    if m < max_v:
                        out.append((cx, cy))
                    m += 1
                qx, qy, q_in = cx, cy, c_in
            poly = out
            if not poly:
                break
        inter_area = f(0.0)
        if poly:
            if len(poly) < 3:
                return 0.0
            s1 = s2 = f(0.0)
            lx, ly = poly[-1]
            for x, y in poly:
                s1 = s1 + x * ly
                s2 = s2 + y * lx
                lx, ly = x, y
            inter_area = f(0.5) * abs(s1 - s2)
            if not inter_area > f(1e-14) * (a1 if a1 > a2 else a2):
                return 0.0
        top = c2[0][1] if c2[0][1] < c1[0][1] else c1[0][1]
        bottom = c2[4][1] if c2[4][1] > c1[4][1] else c1[4][1]
        h = top - bottom
        inter_vol = inter_area * (h if h > 0 else f(0.0))
        v1 = (edge(c1, 0, 1) * edge(c1, 1, 2)) * edge(c1, 0, 4)
        v2 = (edge(c2, 0, 1) * edge(c2, 1, 2)) * edge(c2, 0, 4)
        uni = (v1 + v2) - inter_vol
        return float(inter_vol / uni) if uni > 0 else 0.0


_PAIR_MEMO = {}


def device_iou(a_f32, b_f32):
    """pair_iou_statement on the canon() of two float32 world boxes (memoised); 0 for a box with a non-finite corner."""
    a, b = np.ascontiguousarray(a_f32, np.float32), np.ascontiguousarray(b_f32, np.float32)
    key = (a.tobytes(), b.tobytes())
    if key not in _PAIR_MEMO:
        ok = np.isfinite(a).all() and np.isfinite(b).all()
        _PAIR_MEMO[key] = pair_iou_statement(T.canon(a), T.canon(b)) if ok else 0.0
    return _PAIR_MEMO[key]


def counts_statement(pred_stores, gt_stores, thresholds=THRESHOLDS, K=K_CARE):
    """parq_f1_counts on per-slot lists of statement stores: (counts (2 + T, K) int64, invalid (2,) int64, [best (count,) float64 per
    slot]).  best[i] = max over same-label predictions of device_iou (ground truth first), 0 without one."""
    T_ = len(thresholds)
    counts, invalid, bests = np.zeros((2 + T_, K), np.int64), np.zeros(2, np.int64), []
    for ps, gs in zip(pred_stores, gt_stores):
        ng, npred = gs["count"], ps["count"]
        best = np.zeros(ng, np.float64)
        for i in range(ng):
            for j in range(npred):
                if ps["labels"][j] == gs["labels"][i]:
                    v = device_iou(gs["corners"][i], ps["corners"][j])
                    if v > best[i]:
                        best[i] = v
        bests.append(best)
        for side, (store, n) in enumerate(((gs, ng), (ps, npred))):
            for lab in store["labels"][:n]:
                if 0 <= lab < K:
                    counts[side, lab] += 1
                else:
                    invalid[side] += 1
        for i in range(ng):
            lab = gs["labels"][i]
            if 0 <= lab < K:
                for t, thr in enumerate(thresholds):
                    if best[i] > thr:
                        counts[2 + t, lab] += 1
    return counts, invalid, bests


def entries_store(entries, max_tracks):
    """F1Calculator entries [class, corners, ...] as a statement store."""
    store = T.empty_store(max_tracks)
    for t, e in enumerate(entries):
        store["labels"][t], store["scores"][t], store["corners"][t] = e[0], e[2], e[1]
    store["count"] = len(entries)
    return store


def host_counts(calc, thresholds=THRESHOLDS, K=K_CARE):
    """(2 + T, K) counts of a host calculator through count_matches, scene by scene (F1Calculator.counts)."""
    out = np.zeros((2 + len(thresholds), K), np.int64)
    for t, thr in enumerate(thresholds):
        gts, preds, tps = calc.counts(thr)
        out[0], out[1], out[2 + t] = [gts[c] for c in range(K)], [preds[c] for c in range(K)], [tps[c] for c in range(K)]
    return out


def random_store(n, max_tracks, seed, labels=None, around=None):
    """A statement store of n boxes in a 3 m room; `around`: another store whose boxes (cycled) these are noisy copies of, so that
    the IoUs spread over (0, 1)."""
    rng = np.random.RandomState(seed)
    store = T.empty_store(max_tracks)
    for t in range(n):
        if around is not None and around["count"] and t % 4 != 3:
            src = t % around["count"]
            store["corners"][t] = around["corners"][src] + rng.normal(0, 0.06, 3).astype(np.float32)
            store["labels"][t] = around["labels"][src] if rng.rand() < 0.8 else rng.randint(0, K_CARE)
        else:
            store["corners"][t] = _yaw_box_corners(rng.uniform(-1.5, 1.5, 3) * np.array([1, 1, 0.3]), rng.uniform(0.25, 0.6, 3),
                                                   rng.uniform(-np.pi, np.pi))
            store["labels"][t] = rng.randint(0, K_CARE)
        store["scores"][t] = 1.0 if around is None else rng.uniform(0.2, 1.0)
    if labels is not None:
        store["labels"][:n] = labels
    store["count"] = n
    return store


def counts_case():
    """Per-slot (prediction, ground-truth) stores of the GPU tier's counts test: 0, 1 and 65 tracks per side in every pairing that
    matters, a class with predictions and no ground truth (7) and the reverse (8), and a ground-truth label outside [0, K)."""
    mt_p, mt_g = 80, 72
    g65 = random_store(65, mt_g, 1)
    g65["labels"][:3] = 8
    g65["labels"][64] = K_CARE                                        # `non-object`: outside the care classes
    p65 = random_store(65, mt_p, 2, around=g65)
    p65["labels"][:2] = 7
    g1 = random_store(1, mt_g, 3)
    p1 = random_store(1, mt_p, 4, around=g1)
    p1["labels"][0] = g1["labels"][0] = 4
    preds = [p65, T.empty_store(mt_p), p1, p1, random_store(65, mt_p, 5), T.empty_store(mt_p)]
    gts = [g65, g1, g1, T.empty_store(mt_g), g1, T.empty_store(mt_g)]
    for store in gts:
        lab = store["labels"][:store["count"]]
        lab[lab == 7] = 2
    for store in preds:
        lab = store["labels"][:store["count"]]
        lab[lab == 8] = 3
    return preds, gts, mt_p, mt_g


# ---- cases of the ground-truth store ----------------------------------------------------------------------------------------------
def gt_store_steps(P):
    """Three steps of two scenes for the raw entry.  P = 5: scene "main" uses four rows with an invalid one in the middle; P = 70: 66
    valid rows (past one wavefront).  Scene "none" has no valid row in step 0 and boxes later.  Later steps repeat boxes with noise,
    so matches, pairs under the threshold and births all occur; labels include 9, outside the care classes; the invalid rows hold
    values that must not be read as boxes."""
    rng = np.random.RandomState(70 + P)
    world = {name: [(_yaw_box_corners(np.array([1.7 * (k % 9), 1.9 * (k // 9), 0.0]), rng.uniform(0.3, 0.6, 3), rng.uniform(-np.pi, np.pi)),
                     int(rng.randint(0, 10))) for k in range(75)] for name in ("main", "none")}
    if P == 5:
        main_rows = [[0, 1, 3, 4], [0, 2, 4], [0, 1, 3, 4]]
    else:
        full = [r for r in range(P) if r not in (7, 20, 33, 64)]
        main_rows = [full, list(range(0, P, 3)), full]
    steps = []
    for t in range(3):
        lab, cor, val = np.zeros((2, P), np.int32), np.zeros((2, P, 8, 3), np.float32), np.zeros((2, P), bool)
        for b, name in enumerate(("main", "none")):
            rows = main_rows[t] if name == "main" else ([] if t == 0 else list(range(1, min(P, 12))))
            for r in rows:
                box, cls = world[name][(r + 2 * t) % 75]
                cor[b, r] = box + rng.normal(0, 0.03 * t, 3).astype(np.float32)
                lab[b, r] = cls
                val[b, r] = True
            junk = ~val[b]
            cor[b, junk] = rng.uniform(-9, 9, (int(junk.sum()), 8, 3))
            lab[b, junk] = -5
        steps.append(dict(scenes=["main", "none"], gt_labels=lab, gt_corners=cor, gt_valid=val))
    return steps


def gt_overflow_step():
    """One scene, 12 far-apart boxes in 14 rows: a store of 4 tracks keeps the first four and drops eight."""
    P = 14
    lab, cor, val = np.zeros((1, P), np.int32), np.zeros((1, P, 8, 3), np.float32), np.ones((1, P), bool)
    val[0, [2, 9]] = False
    for k, r in enumerate(np.nonzero(val[0])[0]):
        cor[0, r] = _yaw_box_corners(np.array([3.0 * k, 0.0, 0.0]), np.array([0.4, 0.3, 0.5]), 0.3 * k)
        lab[0, r] = k % 9
    return dict(scenes=["full"], gt_labels=lab, gt_corners=cor, gt_valid=val)


def g12_steps():
    return with_padded_gt(T.g12_steps())


def duplicate_steps():
    return with_padded_gt(E.duplicate_name_steps())
