"""The rule of parq_average_precision (include/parq_hip.h) as a NumPy statement, an independent sequential formulation of the same
metric, and the cases of its tests (test_average_precision_cpu.py, test_gpu_average_precision.py).

The reference's evaluator has no AP, so no reference vector exists: ``ap_statement`` spells the header's rule out, operation by
operation (the order-free true-positive test, the cumulative counts, the running maximum from the right, the float64 sum over the
true-positive ranks in DESCENDING rank, one division), and the kernels must reproduce it exactly.  ``ap_sequential`` is the
textbook PASCAL-VOC / VoteNet evaluation (sort by score, walk, a ``taken`` set, ``mrec`` / ``mpre``) and shares no code with it;
the two differ only in how the recall steps are rounded.  Both read the statement stores of scene_tracks_cases.py and take their
IoUs from f1_device_cases.device_iou (ground truth first: parq_f1_counts's matrix).
"""
import numpy as np

import f1_device_cases as F
import scene_tracks_cases as T
from oracle.make_golden import _yaw_box_corners

THRESHOLDS = (0.25, 0.5)
K_CARE = F.K_CARE


# ---- the statement ------------------------------------------------------------------------------------------------------------------
def score_keys(scores_f32):
    b = np.ascontiguousarray(scores_f32, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b >> np.uint64(31), b ^ np.uint64(0xFFFFFFFF), b ^ np.uint64(0x80000000))


def valid_count(store):
    n, cap = int(store["count"]), len(store["labels"])
    return n if 0 <= n <= cap else 0


def ap_statement(pred_stores, gt_stores, thresholds=THRESHOLDS, K=K_CARE):
    """parq_average_precision on per-slot lists of statement stores.  Returns a dict: ap (T, K) float64, counts (2, K) int64,
    invalid (2,) int64, order (N,) int32, class_start (K + 1,) int32, cum_tp (T, N) int32, pred_best / pred_target (per slot, the
    first `count` rows), flags (T, ranked) bool in rank order, pairs (IoUs evaluated)."""
    S, Tn = len(pred_stores), len(thresholds)
    cap = len(pred_stores[0]["labels"]) if S else 0
    N = S * cap
    counts, invalid = np.zeros((2, K), np.int64), np.zeros(2, np.int64)
    bests, targets, ranked, pairs = [], [], [], 0
    for s, (ps, gs) in enumerate(zip(pred_stores, gt_stores)):
        ng, npred = valid_count(gs), valid_count(ps)
        for lab in gs["labels"][:ng]:
            if 0 <= lab < K:
                counts[0, lab] += 1
            else:
                invalid[0] += 1
        keys = score_keys(ps["scores"])
        best, target = np.zeros(npred, np.float64), -np.ones(npred, np.int32)
        for p in range(npred):
            c = int(ps["labels"][p])
            if not (0 <= c < K) or np.isnan(ps["scores"][p]):
                invalid[1] += 1
                continue
            counts[1, c] += 1
            seen, m = False, 0.0
            for i in range(ng):
                if gs["labels"][i] != c:
                    continue
                v = F.device_iou(gs["corners"][i], ps["corners"][p])
                pairs += 1
                if (not seen and v == v) or (seen and v > m):
                    seen, m, target[p] = True, v, i
            best[p] = m if target[p] >= 0 else 0.0
            ranked.append((c, 0xFFFFFFFF - int(keys[p]), s, p))               # class, score key descending, slot, position
        bests.append(best)
        targets.append(target)
    ranked.sort()
    n = len(ranked)
    order, class_start = -np.ones(N, np.int32), np.zeros(K + 1, np.int32)
    for r, (c, _, s, p) in enumerate(ranked):
        order[r] = s * cap + p
        class_start[c + 1:] += 1
    # the order-free true-positive test, as the header writes it
    flags = np.zeros((Tn, n), bool)
    for t, thr in enumerate(thresholds):
        for r, (c, _, s, p) in enumerate(ranked):
            if targets[s][p] < 0 or not bests[s][p] > thr:
                continue
            earlier = any(s2 == s and targets[s][q] == targets[s][p] and bests[s][q] > thr for _, _, s2, q in ranked[class_start[c]:r])
            flags[t, r] = not earlier
    ap, cum_tp = np.zeros((Tn, K), np.float64), np.zeros((Tn, N), np.int32)
    for t in range(Tn):
        for c in range(K):
            lo, hi = int(class_start[c]), int(class_start[c + 1])
            nn, npos = hi - lo, int(counts[0, c])
            tp = 0
            prec = np.zeros(nn, np.float64)
            for r in range(nn):
                tp += int(flags[t, lo + r])
                cum_tp[t, lo + r] = tp
                prec[r] = np.float64(tp) / np.float64(r + 1)
            pmax = prec.copy()
            for r in range(nn - 2, -1, -1):
                if pmax[r + 1] > pmax[r]:
                    pmax[r] = pmax[r + 1]
            acc = np.float64(0.0)
            for r in range(nn - 1, -1, -1):                                   # descending rank, one add per true positive
                if flags[t, lo + r]:
                    acc = acc + pmax[r]
            ap[t, c] = acc / np.float64(npos) if (npos > 0 and nn > 0) else 0.0
    return dict(ap=ap, counts=counts, invalid=invalid, order=order, class_start=class_start, cum_tp=cum_tp, pred_best=bests,
                pred_target=targets, flags=flags, pairs=pairs)


# ---- the sequential formulation: nothing above is used ---------------------------------------------------------------------------------
def ap_sequential(pred_stores, gt_stores, thresholds=THRESHOLDS, K=K_CARE):
    """Textbook evaluation.  Returns (ap (T, K), per class the detection list [(slot, position)] in walk order, per (t, class) the
    list of true-positive marks in walk order)."""
    dets = {c: [] for c in range(K)}
    npos = {c: 0 for c in range(K)}
    for s, (ps, gs) in enumerate(zip(pred_stores, gt_stores)):
        cnt_g = gs["count"] if 0 <= gs["count"] <= len(gs["labels"]) else 0
        cnt_p = ps["count"] if 0 <= ps["count"] <= len(ps["labels"]) else 0
        for i in range(cnt_g):
            if gs["labels"][i] in npos:
                npos[int(gs["labels"][i])] += 1
        for j in range(cnt_p):
            sc = float(ps["scores"][j])
            if int(ps["labels"][j]) in dets and not np.isnan(sc):
                zero_sign = 1 if (sc == 0.0 and np.signbit(sc)) else 0      # -0.0 behind +0.0
                dets[int(ps["labels"][j])].append((-sc, zero_sign, s, j))
    ap = np.zeros((len(thresholds), K), np.float64)
    walks, marks = {}, {}
    for c in range(K):
        walk = sorted(dets[c])
        walks[c] = [(s, j) for _, _, s, j in walk]
        for t, thr in enumerate(thresholds):
            taken = set()
            tp, fp = np.zeros(len(walk)), np.zeros(len(walk))
            for d, (_, _, s, j) in enumerate(walk):
                gs, ps = gt_stores[s], pred_stores[s]
                cnt_g = gs["count"] if 0 <= gs["count"] <= len(gs["labels"]) else 0
                cand = [i for i in range(cnt_g) if gs["labels"][i] == c]
                ious = np.array([F.device_iou(gs["corners"][i], ps["corners"][j]) for i in cand], np.float64)
                ious = np.where(np.isnan(ious), -np.inf, ious)
                hit = False
                if len(cand) and np.isfinite(ious.max()):
                    k = int(np.argmax(ious))                                # numpy returns the first maximum
                    if ious[k] > thr and (s, cand[k]) not in taken:
                        taken.add((s, cand[k]))
                        hit = True
                tp[d], fp[d] = hit, not hit
            marks[t, c] = tp.astype(bool).tolist()
            if npos[c] == 0 or len(walk) == 0:
                continue
            ctp, cfp = np.cumsum(tp), np.cumsum(fp)
            rec, prec = ctp / npos[c], ctp / (ctp + cfp)
            mrec, mpre = np.concatenate([[0.0], rec, [1.0]]), np.concatenate([[0.0], prec, [0.0]])
            for i in range(len(mpre) - 1, 0, -1):
                mpre[i - 1] = max(mpre[i - 1], mpre[i])
            idx = np.nonzero(mrec[1:] != mrec[:-1])[0]
            ap[t, c] = float(np.sum((mrec[idx + 1] - mrec[idx]) * mpre[idx + 1]))
    return ap, walks, marks


# ---- stores on the device -------------------------------------------------------------------------------------------------------------
def store_row(store, mt):
    """A statement store as the (2 + 26 * mt) int32 words of a slot."""
    row = np.zeros(2 + 26 * mt, np.int32)
    row[0], row[1] = store["count"], store["dropped"]
    row[2:2 + mt] = store["labels"]
    row[2 + mt:2 + 2 * mt] = np.ascontiguousarray(store["scores"], np.float32).view(np.int32)
    row[2 + 2 * mt:] = np.ascontiguousarray(store["corners"], np.float32).reshape(-1).view(np.int32)
    return row


def store_words(stores, mt):
    return np.stack([store_row(s, mt) for s in stores]) if stores else np.zeros((0, 2 + 26 * mt), np.int32)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def scored_counts_case(seed=11):
    """f1_device_cases.counts_case() (0, 1 and 65 tracks per side, an out-of-range ground-truth label) with seeded random scores,
    some of them equal."""
    preds, gts, mt_p, mt_g = F.counts_case()
    rng = np.random.RandomState(seed)
    preds = [dict(p, scores=p["scores"].copy()) for p in preds]
    for p in preds:
        p["scores"][:p["count"]] = (rng.randint(1, 40, p["count"]) / 40.0).astype(np.float32)
    return preds, gts, mt_p, mt_g


def random_case(seed, scenes=4):
    """Seeded random stores: up to 13 ground-truth and 19 prediction tracks per scene, the predictions noisy copies."""
    rng = np.random.RandomState(300 + seed)
    preds, gts = [], []
    for s in range(scenes):
        g = F.random_store(int(rng.randint(0, 14)), 16, 20 * seed + s)
        p = F.random_store(int(rng.randint(0, 20)), 24, 500 + 20 * seed + s, around=g)
        p["scores"][:p["count"]] = np.round(p["scores"][:p["count"]], 1 + seed % 2)        # equal scores within and across scenes
        gts.append(g)
        preds.append(p)
    return preds, gts


def _cube(x, y=0.0):
    return _yaw_box_corners(np.array([x, y, 0.0]), (0.5, 0.5, 0.5), 0.0).astype(np.float32)


def _fill(mt, rows):
    """rows: [(label, x, score)] -> a statement store; unit cubes shifted along x (IoU of a shift d: (1 - d) / (1 + d))."""
    store = T.empty_store(mt)
    for k, (lab, x, score) in enumerate(rows):
        store["labels"][k], store["corners"][k], store["scores"][k] = lab, _cube(x), score
    store["count"] = len(rows)
    return store


HAND_THRESHOLDS = (0.1, 0.25, 0.5)
HAND_MT_P, HAND_MT_G = 12, 9


def hand_case():
    """Two scenes, every sub-case in a class of its own.  Returns (preds, gts, expected): expected["flags"][(slot, position)] = the
    true-positive marks at HAND_THRESHOLDS of every ranked prediction, expected["order"] the ranks as (slot, position),
    expected["ap"] (T, K), expected["invalid"], expected["counts"].
      class 0: prediction 1's arg-max box (IoU 0.538) is claimed by prediction 0; its second-best box (0.176 > 0.1) is free: still false.
      class 3: two claimants of one box; the higher-scored one has IoU 1/3: it wins at 0.1 and 0.25 and loses the box at 0.5.
      class 1: equal scores within a scene (position decides) and across scenes (slot decides).
      class 2: scores -0.0 and +0.0: +0.0 is ranked first.
      class 4: a NaN score (not ranked).  Labels 9 and -1 on the ground-truth side, 9 on the prediction side.
      class 7: predictions and no ground truth; class 8: the reverse."""
    nan = np.float32(np.nan)
    g0 = _fill(HAND_MT_G, [(0, 0.0, 1), (0, 1.0, 1), (3, 0.0, 1), (1, 0.0, 1), (2, 0.0, 1), (9, 0.0, 1), (8, 0.0, 1), (-1, 0.0, 1)])
    p0 = _fill(HAND_MT_P, [(0, 0.1, 0.9), (0, 0.3, 0.8), (3, 0.5, 0.9), (3, 0.1, 0.8), (1, 0.1, 0.5), (1, 0.05, 0.5), (2, 0.05, -0.0),
                           (2, 0.1, 0.0), (4, 0.0, nan), (9, 0.0, 0.9), (7, 0.0, 0.7)])
    g1 = _fill(HAND_MT_G, [(1, 0.0, 1), (8, 5.0, 1)])
    p1 = _fill(HAND_MT_P, [(1, 0.2, 0.5), (7, 0.0, 0.7)])
    assert np.signbit(p0["scores"][6]) and not np.signbit(p0["scores"][7])
    yes, no = (True, True, True), (False, False, False)
    flags = {(0, 0): yes, (0, 1): no, (0, 2): (True, True, False), (0, 3): (False, False, True), (0, 4): yes, (0, 5): no, (0, 6): no,
             (0, 7): yes, (0, 10): no, (1, 0): yes, (1, 1): no}
    order = [(0, 0), (0, 1), (0, 4), (0, 5), (1, 0), (0, 7), (0, 6), (0, 2), (0, 3), (0, 10), (1, 1)]
    ap = np.zeros((3, K_CARE))
    ap[:, 0] = 0.5                            # TP FP, two boxes
    ap[:, 1] = (2.0 / 3.0 + 1.0) / 2.0        # TP FP TP, two boxes: pmax 1, 2/3, 2/3, summed from the last rank
    ap[:, 2] = 1.0
    ap[:2, 3], ap[2, 3] = 1.0, 0.5            # TP FP, then FP TP
    counts = np.zeros((2, K_CARE), np.int64)
    counts[0, [0, 1, 2, 3, 8]] = 2, 2, 1, 1, 2
    counts[1, [0, 1, 2, 3, 7]] = 2, 3, 2, 2, 2
    return [p0, p1], [g0, g1], dict(flags=flags, order=order, ap=ap, invalid=[2, 2], counts=counts)


SORT_S, SORT_MT_P, SORT_MT_G = 9, 600, 4


def sort_case():
    """9 scenes at prediction capacity 600: 5400 positions (padded to 8192: four LDS tiles of 2048), about 5000 ranked predictions
    with many equal scores; class 2's segment lies across rank 2048 and class 5's across rank 4096.  Ground truth exists in four
    scenes only, one to four boxes each, so the statement evaluates under a couple of thousand pairs."""
    rng = np.random.RandomState(77)
    gt_of = {0: [(7, 0.0), (7, 2.0)], 3: [(2, 0.0), (2, 2.0), (2, 4.0), (2, 6.0)], 5: [(5, 0.0), (5, 2.0), (5, 4.0), (5, 6.0)], 8: [(0, 0.0)]}
    base = _cube(0.0)
    preds, gts = [], []
    for s in range(SORT_S):
        g = _fill(SORT_MT_G, [(lab, x, 1) for lab, x in gt_of.get(s, [])])
        n = 540 + 7 * s
        p = T.empty_store(SORT_MT_P)
        p["labels"][:n] = rng.choice([0, 2, 5, 7], size=n, p=[0.3, 0.3, 0.3, 0.1])
        p["scores"][:n] = (rng.randint(0, 200, n) / 200.0).astype(np.float32)
        shift = np.zeros((n, 1, 3), np.float32)
        shift[:, 0, 0] = rng.choice([0.05, 0.1, 0.4, 2.05, 2.2, 4.1, 6.3, 9.0], size=n)
        p["corners"][:n] = base[None] + shift
        p["labels"][n - 1] = 11                                               # not ranked, in the middle of the position range
        p["scores"][n - 2] = np.nan
        p["count"] = n
        gts.append(g)
        preds.append(p)
    return preds, gts
