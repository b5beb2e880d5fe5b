"""CPU tier of the average precision (include/parq_hip.h parq_average_precision; parq_amd/f1_eval.py average_precision_host): the
NumPy statement of tests/average_precision_cases.py against an independent sequential formulation, the metric's properties, the
hand-made cases with their expected marks written out, the entry points' declaration and binding, the refusals that return before
any device call, and the host calculator with the flag on.  The reference's evaluator has no AP: there is no reference vector."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import parq_amd
from parq_amd import _lib, f1_eval
from parq_amd.f1_eval import F1Calculator
from parq_amd.scene_tracks import SceneTracks, average_precision, check_average_precision_args

import average_precision_cases as A
import eval_iou_cases as E
import f1_device_cases as F
import scene_tracks_cases as T
from oracle.make_golden import F1_CASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"parq_average_precision_workspace_bytes": ["S", "pred_max_tracks", "gt_max_tracks", "T", "K"],
       "parq_average_precision": ["pred_store", "pred_max_tracks", "gt_store", "gt_max_tracks", "S", "thresholds_host", "T", "K", "workspace",
                                  "workspace_bytes", "ap", "counts", "invalid", "order", "class_start", "cum_tp", "pred_best", "pred_target",
                                  "stream"]}


def _ranks(res, cap):
    """The statement's filled ranks as (slot, position)."""
    n = int(res["class_start"][-1])
    assert (res["order"][n:] == -1).all() and (res["order"][:n] >= 0).all()
    return [(int(o) // cap, int(o) % cap) for o in res["order"][:n]]


def _assert_equals_sequential(preds, gts, thresholds, K=A.K_CARE):
    res = A.ap_statement(preds, gts, thresholds, K)
    ap, walks, marks = A.ap_sequential(preds, gts, thresholds, K)
    cap = len(preds[0]["labels"])
    ranks, cs = _ranks(res, cap), res["class_start"]
    for c in range(K):
        assert ranks[cs[c]:cs[c + 1]] == walks[c], c                           # the order, exactly
        for t in range(len(thresholds)):
            assert res["flags"][t, cs[c]:cs[c + 1]].tolist() == marks[t, c], (t, c)     # the marks, exactly
            assert res["cum_tp"][t, cs[c]:cs[c + 1]].tolist() == np.cumsum(marks[t, c]).astype(int).tolist(), (t, c)
    worst = float(np.abs(res["ap"] - ap).max())
    assert worst <= 1e-12, worst                                             # the recall steps are rounded differently, nothing else
    return res, worst


# ---- the statement against the sequential formulation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_statement_equals_the_sequential_formulation_on_random_cases(seed):
    preds, gts = A.random_case(seed)
    res, worst = _assert_equals_sequential(preds, gts, (0.1, 0.25, 0.5, 0.7))
    print("seed %d: %d ranked, %d true positives at 0.25, max |statement - sequential| = %.3e"
          % (seed, res["class_start"][-1], res["flags"][1].sum(), worst))
    assert res["flags"][1].sum() > res["flags"][3].sum() > 0 and res["flags"][0].sum() < res["class_start"][-1]
    assert 0 < res["ap"].max() <= 1.0 and res["ap"].min() >= 0.0


def test_statement_equals_the_sequential_formulation_on_the_scored_counts_case():
    preds, gts, mt_p, mt_g = A.scored_counts_case()
    res, _ = _assert_equals_sequential(preds, gts, A.THRESHOLDS)
    assert res["invalid"].tolist() == [1, 0] and res["pairs"] < 2000
    # equal scores occur, within a scene and across scenes
    keys = [(int(p["labels"][j]), float(p["scores"][j])) for p in preds for j in range(p["count"])]
    assert len(set(keys)) < len(keys)


# ---- properties -----------------------------------------------------------------------------------------------------------------------
def test_predictions_equal_to_the_ground_truth_give_ap_one_whatever_their_scores():
    """Equal as the evaluator sees it: the ground truth is stored moved by its jitter (a box clipped against its exact copy has
    every vertex ON an edge, and the strict inside test of the reference's routine then decides by rounding)."""
    _, gts = A.random_case(5)
    rng = np.random.RandomState(0)
    preds = []
    for s, g in enumerate(gts):
        p = T.empty_store(16)
        n = g["count"]
        p["labels"][:n], p["corners"][:n], p["count"] = g["labels"][:n], g["corners"][:n], n
        p["scores"][:n] = rng.uniform(-1, 1, n).astype(np.float32)
        g["corners"][:n] = F.jittered(g["corners"][:n], F.gt_jitter(3, s, 0, np.arange(n)))
        preds.append(p)
    res = A.ap_statement(preds, gts, (0.25, 0.5, 0.7))
    have = res["counts"][0] > 0
    assert have.sum() >= 5 and (res["ap"][:, have] == 1.0).all() and (res["ap"][:, ~have] == 0.0).all()


def test_a_monotone_rescoring_changes_nothing():
    preds, gts = A.random_case(1)
    base = A.ap_statement(preds, gts)
    again = A.ap_statement([dict(p, scores=p["scores"] * np.float32(0.5)) for p in preds], gts)     # exact in float32
    cubed = A.ap_statement([dict(p, scores=(p["scores"].astype(np.float64) ** 3).astype(np.float32)) for p in preds], gts)
    for other in (again, cubed):
        assert np.array_equal(other["order"], base["order"]) and np.array_equal(other["flags"], base["flags"])
        assert np.array_equal(other["ap"].view(np.int64), base["ap"].view(np.int64))


def test_a_lowest_scored_false_positive_appended_changes_no_ap():
    preds, gts = A.random_case(2)
    base = A.ap_statement(preds, gts)
    c = int(np.argmax(base["ap"][0]))
    more = [dict(p, labels=p["labels"].copy(), scores=p["scores"].copy(), corners=p["corners"].copy()) for p in preds]
    n = more[0]["count"]
    more[0]["labels"][n], more[0]["scores"][n], more[0]["corners"][n], more[0]["count"] = c, -5.0, A._cube(40.0), n + 1
    res = A.ap_statement(more, gts)
    assert res["counts"][1, c] == base["counts"][1, c] + 1
    assert np.array_equal(res["ap"].view(np.int64), base["ap"].view(np.int64)) and base["ap"][0, c] > 0


@pytest.mark.parametrize("seed", [0, 3])
def test_true_positives_and_best_ious_are_bounded_by_the_f1_counts(seed):
    preds, gts = A.random_case(seed)
    thresholds = (0.25, 0.5, 0.7)
    res = A.ap_statement(preds, gts, thresholds)
    counts, invalid, gt_best = F.counts_statement(preds, gts, thresholds)
    cs = res["class_start"]
    assert np.array_equal(res["counts"], counts[:2]) and np.array_equal(res["invalid"], invalid)
    for t in range(3):
        for c in range(A.K_CARE):
            final = int(res["cum_tp"][t, cs[c + 1] - 1]) if cs[c + 1] > cs[c] else 0
            assert final <= counts[2 + t, c], (t, c)                         # a claimed box is a matched box, not the other way round
    # one IoU matrix: per scene and class its maximum, seen from either side
    for s, (p, g) in enumerate(zip(preds, gts)):
        for c in range(A.K_CARE):
            from_pred = max([res["pred_best"][s][j] for j in range(p["count"]) if p["labels"][j] == c], default=0.0)
            from_gt = max([gt_best[s][i] for i in range(g["count"]) if g["labels"][i] == c], default=0.0)
            assert from_pred == from_gt, (s, c)


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------
def test_hand_made_cases_give_the_marks_written_out():
    preds, gts, want = A.hand_case()
    res = A.ap_statement(preds, gts, A.HAND_THRESHOLDS)
    ranks = _ranks(res, A.HAND_MT_P)
    assert ranks == want["order"]
    for r, sp in enumerate(ranks):
        assert tuple(bool(res["flags"][t, r]) for t in range(3)) == want["flags"][sp], sp
    assert res["invalid"].tolist() == want["invalid"] and np.array_equal(res["counts"], want["counts"])
    assert np.array_equal(res["ap"], want["ap"]), (res["ap"], want["ap"])
    # the geometry is what the docstring says
    b, tg = res["pred_best"][0], res["pred_target"][0]
    assert abs(b[1] - 0.7 / 1.3) < 1e-6 and tg[1] == 0 and abs(F.device_iou(gts[0]["corners"][1], preds[0]["corners"][1]) - 0.3 / 1.7) < 1e-6
    assert 0.25 < b[2] < 0.5 < b[3] and tg[2] == tg[3] == 2
    assert tg[8] == -1 and tg[9] == -1 and tg[10] == -1 and b[10] == 0.0       # NaN score, label 9, no same-class ground truth
    _assert_equals_sequential(preds, gts, A.HAND_THRESHOLDS)
    # all IoUs zero: the target is the first same-class box
    far = [A._fill(4, [(0, 50.0, 0.5)])]
    res = A.ap_statement(far, [A._fill(4, [(1, 0.0, 1), (0, 0.0, 1), (0, 1.0, 1)])], (0.25,))
    assert res["pred_target"][0].tolist() == [1] and res["pred_best"][0].tolist() == [0.0] and not res["flags"].any()


def test_host_statement_is_the_statement_on_entry_lists():
    for preds, gts, thresholds in (A.hand_case()[:2] + (A.HAND_THRESHOLDS,), A.random_case(1) + (A.THRESHOLDS,)):
        want = A.ap_statement(preds, gts, thresholds)
        ent_p = [[[int(p["labels"][j]), p["corners"][j], p["scores"][j], j] for j in range(p["count"])] for p in preds]
        ent_g = [[(int(g["labels"][i]), g["corners"][i], 1) for i in range(g["count"])] for g in gts]
        got = f1_eval.average_precision_host(ent_p, ent_g, thresholds, A.K_CARE, pair_iou=F.device_iou)
        cap = len(preds[0]["labels"])
        assert got["order"] == _ranks(want, cap) and np.array_equal(got["class_start"], want["class_start"])
        n = len(got["order"])
        assert np.array_equal(got["cum_tp"], want["cum_tp"][:, :n])
        assert np.array_equal(got["ap"].view(np.int64), want["ap"].view(np.int64))
        assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["invalid"], want["invalid"])
        for s in range(len(preds)):
            assert np.array_equal(got["best"][s], want["pred_best"][s]) and np.array_equal(got["target"][s], want["pred_target"][s])
        # the host routine's IoU moves no decision here
        host = f1_eval.average_precision_host(ent_p, ent_g, thresholds, A.K_CARE)
        assert np.array_equal(host["ap"].view(np.int64), want["ap"].view(np.int64))
    assert f1_eval.score_key(np.float32(0.0)) == int(A.score_keys(np.zeros(1, np.float32))[0]) == 0x80000000
    assert f1_eval.score_key(np.float32(-0.0)) == 0x7FFFFFFF and f1_eval.score_key(np.float32(-1.0)) < f1_eval.score_key(np.float32(-0.5))


def test_sort_case_holds_what_its_docstring_says():
    preds, gts = A.sort_case()
    assert len(preds) == 9 and all(len(p["labels"]) == 600 for p in preds) and 9 * 600 == 5400
    labels = np.concatenate([p["labels"][:p["count"]] for p in preds])
    scores = np.concatenate([p["scores"][:p["count"]] for p in preds])
    ranked = (labels >= 0) & (labels < A.K_CARE) & ~np.isnan(scores)
    start = np.concatenate([[0], np.cumsum(np.bincount(labels[ranked], minlength=A.K_CARE))])
    assert start[2] < 2048 < start[3] and start[5] < 4096 < start[6] and 4900 < start[-1] < 5400
    pairs = sum(int((p["labels"][:p["count"]][ranked_s] == lab).sum()) for p, g in zip(preds, gts) for lab in g["labels"][:g["count"]]
                for ranked_s in [~np.isnan(p["scores"][:p["count"]])])
    assert 500 < pairs < 2000


# ---- header, binding, exports ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_binding_types_them():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    for name, names in NEW.items():
        m = re.search(r"\b(?:int|size_t)\s+\(%s\)\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/parq_hip.h must declare %s with a parenthesised name" % name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names, name
        assert name in _lib.AP_SYMBOLS and not any(name in t for t in _lib.ALL_TABLES + (_lib.EVAL_SYMBOLS, _lib.LIFE_SYMBOLS))
        res, args = _lib.AP_SYMBOLS[name]
        assert len(args) == len(names) and res is (C.c_size_t if name.endswith("bytes") else C.c_int)
    assert len(_lib.AP_SYMBOLS) == 2 and _lib.AP_SYMBOLS not in _lib.ALL_TABLES
    for phrase in ("DESCENDING rank", "b ^ ((b >> 31) ? 0xffffffff : 0x80000000)", "no reference vector"):
        assert phrase in hdr, phrase
    from parq_amd import scene_tracks
    assert parq_amd.average_precision is average_precision is scene_tracks.average_precision
    from parq_amd.decoder import PARQDecoder
    assert PARQDecoder.average_precision is False and F1Calculator(0.1).average_precision is False
    src = open(os.path.join(ROOT, "parq_amd", "csrc", "avg_precision.hip")).read()
    assert '#include "obb_pair.hpp"' in src and not re.search(r"atomic\w*\s*\(", src) and "hipMalloc" not in src


def test_library_exports_the_entry_points_and_sizes():
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.AP_SYMBOLS[name][1] and fn.restype is _lib.AP_SYMBOLS[name][0]
    w = lib.parq_average_precision_workspace_bytes
    # the padded keys, a maximum, a target and a flag byte per position, and the cumulative counts per threshold
    assert w(9, 600, 4, 2, 9) >= 8192 * 8 + 5400 * (8 + 4 + 1 + 2 * 4) and w(9, 600, 4, 2, 9) % 16 == 0
    assert w(512, 2048, 8, 1, 1) > 0 and w(0, 8, 8, 2, 9) < 256
    for bad in ((-1, 8, 8, 2, 9), (65536, 8, 8, 2, 9), (1, 0, 8, 2, 9), (1, 2049, 8, 2, 9), (1, 8, 0, 2, 9), (1, 8, 2049, 2, 9), (1, 8, 8, 0, 9),
                (1, 8, 8, 9, 9), (1, 8, 8, 2, 0), (1, 8, 8, 2, 33), (513, 2048, 8, 2, 9), (65535, 17, 8, 2, 9)):
        assert w(*bad) == 0, bad


def test_argument_errors_return_before_any_device_call():
    """PARQ_ERR_ARG (1) from checks made on the host: the pointers below are never dereferenced."""
    lib = _lib.load()
    p, odd = C.c_void_p(4096), C.c_void_p(4104)
    thr = (C.c_double * 2)(0.25, 0.5)
    need = lib.parq_average_precision_workspace_bytes(2, 8, 8, 2, 9)
    assert need > 0

    def f(ps=p, pm=8, gs=p, gm=8, S=2, th=thr, T=2, K=9, ws=p, wsb=need, ap=p, counts=p, invalid=p, opt=(None,) * 5):
        return lib.parq_average_precision(ps, pm, gs, gm, S, th, T, K, ws, wsb, ap, counts, invalid, *opt, None)
    bad_cases = [dict(S=-1), dict(S=65536), dict(pm=0), dict(pm=2049), dict(gm=0), dict(gm=2049), dict(T=0), dict(T=9), dict(K=0), dict(K=33),
                 dict(S=513, pm=2048), dict(ps=None), dict(gs=None), dict(th=None), dict(ws=None), dict(ap=None), dict(counts=None),
                 dict(invalid=None), dict(wsb=need - 1), dict(ws=odd)]
    for k in range(5):                                                        # optional outputs given only in part
        bad_cases.append(dict(opt=tuple(p if i == k else None for i in range(5))))
        bad_cases.append(dict(opt=tuple(None if i == k else p for i in range(5))))
        bad_cases.append(dict(S=0, opt=tuple(None if i == k else p for i in range(5))))
    for bad in bad_cases:
        assert f(**bad) == 1, bad
    assert b"parq_average_precision" in lib.parq_last_error()


def test_python_surface_checks_its_arguments_before_the_gpu():
    a, b = SceneTracks(max_tracks=8), SceneTracks(max_tracks=8)
    assert check_average_precision_args(a, b, [0.25, 0.5], 9) == ([0.25, 0.5], 0)
    with pytest.raises(TypeError):
        average_precision(None, None, [0.5])
    with pytest.raises(TypeError):
        average_precision(a, None, [0.5])
    with pytest.raises(ValueError, match="thresholds"):
        average_precision(a, b, [])
    with pytest.raises(ValueError, match="thresholds"):
        average_precision(a, b, [0.1] * 9)
    for k in (0, 33, True, 9.0):
        with pytest.raises(ValueError, match="num_classes"):
            average_precision(a, b, [0.5], num_classes=k)
    a._slots = {"x": 0}
    with pytest.raises(ValueError, match="same scenes"):
        average_precision(a, b, [0.5])
    big_a, big_b = SceneTracks(max_tracks=2048), SceneTracks(max_tracks=2048)
    big_a._slots = big_b._slots = {k: k for k in range(513)}
    with pytest.raises(ValueError, match="positions"):
        average_precision(big_a, big_b, [0.5])


# ---- the host calculator ------------------------------------------------------------------------------------------------------------
def test_host_calculator_adds_the_ap_keys_and_keeps_the_nine_metrics_of_the_golden():
    calc = F1Calculator(F1_CASE["conf"], average_precision=True)
    metrics = E.run_g12(calc)
    nine = {k: v for k, v in metrics.items() if "AP" not in k}
    E.assert_g12(calc, nine)                                                  # tracks, ids, scores and the nine metrics unchanged
    plain = F1Calculator(F1_CASE["conf"])
    assert E.run_g12(plain) == nine and set(plain.compute_metrics()) == set(nine)          # the flag off: exactly today's keys
    extra = {k: v for k, v in metrics.items() if "AP" in k}
    assert set(extra) == {"%s_%s" % (t, k) for t in (0.25, 0.5, 0.7) for k in ["mAP"] + ["AP_" + n for n in f1_eval.CARE_CLASSES.values()]}
    # ... equal to the statement on the calculator's own track lists
    names = list(calc.preds)
    res = A.ap_statement([F.entries_store(calc.preds[n], 64) for n in names], [F.entries_store(calc.gts[n], 64) for n in names], (0.25, 0.5, 0.7))
    have = [c for c in range(9) if res["counts"][0, c] > 0]
    assert len(have) >= 3 and res["ap"].max() > 0
    for t, thr in enumerate((0.25, 0.5, 0.7)):
        for c, name in f1_eval.CARE_CLASSES.items():
            assert extra["%s_AP_%s" % (thr, name)] == res["ap"][t, c], (thr, name)
        total = 0.0
        for c in have:
            total = total + float(res["ap"][t, c])
        assert extra["%s_mAP" % thr] == total / len(have)
    empty = F1Calculator(0.1, average_precision=True).compute_metrics()
    assert len(empty) == 9 + 3 * 10 and all(v == 0 for v in empty.values())
