"""CPU tier of the evaluator's device path (include/parq_hip.h parq_gt_tracks_update / parq_f1_counts; parq_amd/f1_eval.py gt_jitter,
gt_store): the NumPy statements of tests/f1_device_cases.py against the host calculator in "hash" mode and against count_matches,
the properties of the hashed jitter, the entry points' declaration and binding, and the argument checks that return before any
device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import parq_amd
from parq_amd import _lib, f1_eval
from parq_amd.f1_eval import F1Calculator
from parq_amd.scene_tracks import SceneTracks, check_labelled_args, f1_counts

import eval_iou_cases as E
import f1_device_cases as F
import scene_tracks_cases as T
from oracle.make_golden import F1_CASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"parq_gt_tracks_update_workspace_bytes": ["B", "P", "max_tracks"],
       "parq_gt_tracks_update": ["store", "S_cap", "max_tracks", "slots_host", "visits_host", "B", "corners_world", "labels", "valid", "P",
                                 "iou_thresh", "seed", "workspace", "workspace_bytes", "iou_out", "stream"],
       "parq_f1_counts_workspace_bytes": ["S", "gt_max_tracks", "T", "K"],
       "parq_f1_counts": ["pred_store", "pred_max_tracks", "gt_store", "gt_max_tracks", "S", "thresholds_host", "T", "K", "workspace",
                          "workspace_bytes", "counts", "invalid", "best_iou", "stream"]}


# ---- the jitter ---------------------------------------------------------------------------------------------------------------
def _keys_100k(seed=0):
    """The jitter of 100 slots x 10 visits x 100 positions."""
    return np.stack([[F.gt_jitter(seed, s, v, np.arange(100)) for v in range(10)] for s in range(100)])


def test_jitter_bounds_mean_and_deviation():
    j = _keys_100k()
    n = j.size
    assert n == 10 ** 5 and j.dtype == np.float64
    assert np.abs(j).max() <= 3.5e-3 and 131070 * F.JITTER_UNIT <= 3.5e-3
    # every value is an integer multiple of the unit: one product of an integer with the stated constant
    u = np.rint(j / F.JITTER_UNIT)
    assert np.array_equal(u * F.JITTER_UNIT, j) and np.abs(u).max() <= 131070
    # a sum of four uniform 16-bit fields: sigma = 1e-3, kurtosis 3 - 1.2 / 4; three standard errors of the mean and of the deviation
    se_mean = 1e-3 / np.sqrt(n)
    se_std = 1e-3 * np.sqrt((2.7 - 1.0) / (4.0 * n))
    print("mean %.3e (3 se = %.3e), std - 1e-3 = %.3e (3 se = %.3e)" % (j.mean(), 3 * se_mean, j.std() - 1e-3, 3 * se_std))
    assert abs(j.mean()) <= 3 * se_mean
    assert abs(j.std() - 1e-3) <= 3 * se_std


def test_jitter_depends_on_every_word_of_its_key():
    j = _keys_100k()
    assert len(np.unique(j[:, 0, 0])) > 95 and len(np.unique(j[0, :, 0])) == 10 and len(np.unique(j[0, 0, :])) > 95
    base = F.gt_jitter(0, 3, 2, np.arange(64))
    for other in (F.gt_jitter(1, 3, 2, np.arange(64)), F.gt_jitter(1 << 32, 3, 2, np.arange(64)), F.gt_jitter(0, 4, 2, np.arange(64)),
                  F.gt_jitter(0, 3, 3, np.arange(64)), F.gt_jitter(0, 3, 2, np.arange(64, 128))):
        assert (other != base).sum() > 60
    assert np.array_equal(F.gt_jitter(0, 3, 2, np.arange(64)), base)


def test_the_calculator_and_the_statement_hold_the_same_jitter():
    for seed, slot, visit in ((0, 0, 0), (7, 3, 2), ((1 << 63) + 12345, 70000, 9)):
        assert np.array_equal(f1_eval.hash_jitter(seed, slot, visit, 130).view(np.int64), F.gt_jitter(seed, slot, visit, np.arange(130)).view(np.int64))
    assert f1_eval.GT_JITTER_UNIT == F.JITTER_UNIT
    c = np.random.RandomState(0).uniform(-4, 4, (5, 8, 3)).astype(np.float32)
    j = F.gt_jitter(0, 0, 0, np.arange(5))
    assert np.array_equal(f1_eval.apply_jitter(c, j), F.jittered(c, j)) and f1_eval.apply_jitter(c, j).dtype == np.float32
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    assert repr(F.JITTER_UNIT) in hdr and "131070" in hdr


def test_default_numpy_mode_is_todays_behaviour_draw_for_draw():
    calc = F1Calculator(F1_CASE["conf"])
    assert (calc.gt_jitter, calc.gt_store, calc.gt_seed) == ("numpy", "host", 0)
    metrics = E.run_g12(calc)
    E.assert_g12(calc, metrics)                                       # tracks, ids, scores and the nine metrics of the golden
    explicit = F1Calculator(F1_CASE["conf"], gt_jitter="numpy")
    E.run_g12(explicit)
    assert E.tracker_state(explicit) == E.tracker_state(calc)
    # the ground-truth store holds make_gt_list's draws: the same seed, the same boxes in the same order
    np.random.seed(F1_CASE["np_seed"])
    first = F1Calculator.make_gt_list([{"labels": torch.from_numpy(x["labels"]), "gt_corners_world": torch.from_numpy(x["corners"])}
                                       for x in T.g12_steps()[0]["gts"]])
    again = F1Calculator(F1_CASE["conf"])
    np.random.seed(F1_CASE["np_seed"])
    E._feed(again, T.g12_steps()[0])
    for name, want in zip(F1_CASE["scenes"], first):
        assert len(again.gts[name]) == len(want)
        for got, w in zip(again.gts[name], want):
            assert got[0] == w[0] and np.array_equal(got[1], w[1])


# ---- the ground-truth statement against the host calculator in "hash" mode ---------------------------------------------------------
def _host_hash_run(steps, seed):
    calc = F.hash_calculator(seed)
    np.random.seed(0)
    state = np.random.get_state()[1].copy()
    for st in steps:
        E._feed(calc, st)
    assert np.array_equal(np.random.get_state()[1], state)            # "hash" draws nothing from NumPy's generator
    return calc


@pytest.mark.parametrize("case", ["g12", "duplicate"])
def test_gt_statement_equals_the_host_calculator_in_hash_mode(case):
    steps = F.g12_steps() if case == "g12" else F.duplicate_steps()
    for seed in (0, 7):
        calc = _host_hash_run(steps, seed)
        stores, trace, slots = F.gt_run_statement(steps, 64, seed=seed)
        assert set(stores) == set(calc.gts) and list(slots) == list(calc._gt_slots)
        for name in stores:
            # births of one step may be ordered differently (never-assigned before under-threshold on the host): a multiset
            assert F.store_multiset(stores[name]) == F.entries_multiset(calc.gts[name]), (seed, name)
            assert stores[name]["dropped"] == 0 and (stores[name]["scores"][:stores[name]["count"]] == 1.0).all()
    other = F.gt_run_statement(steps, 64, seed=8)[0]
    assert any(F.store_multiset(other[n]) != F.store_multiset(stores[n]) for n in stores)


def test_g12_in_hash_mode_keeps_the_prediction_tracks_and_the_gt_counts_of_the_golden():
    calc = _host_hash_run(F.g12_steps(), 0)
    g = E.g12()
    for name in F1_CASE["scenes"]:
        assert len(calc.preds[name]) == int(g["ntrack_" + name])
        assert np.array_equal([t[0] for t in calc.preds[name]], g["trackcls_" + name])
        assert np.array_equal([t[-1] for t in calc.preds[name]], g["trackid_" + name])
        assert np.array_equal(np.array([t[2] for t in calc.preds[name]], np.float64), g["trackscore_" + name])
    assert [len(calc.gts[n]) for n in F1_CASE["scenes"]] == [int(g["ngt_" + n]) for n in F1_CASE["scenes"]] == [6, 7, 6]
    calc.reset()
    assert calc._gt_slots == {} and calc._gt_visits == {} and calc.gts == {}


def test_padded_ground_truth_is_the_list_form():
    steps = F.g12_steps()
    want = _host_hash_run(steps, 3)
    calc = F.hash_calculator(3)
    for st in steps:
        out = {"pred_corners_world": torch.from_numpy(st["corners"]), "sem_cls_prob": torch.from_numpy(st["prob"]),
               "pred_mask": torch.from_numpy(st["mask"]), "scene_name": st["scenes"]}
        calc.step(out, {"labels": torch.from_numpy(st["gt_labels"]), "gt_corners_world": torch.from_numpy(st["gt_corners"]),
                        "valid": torch.from_numpy(st["gt_valid"])})
    assert E.tracker_state(calc) == E.tracker_state(want)


def test_pair_iou_statement_is_the_host_routine_within_its_own_bound():
    """obb_pair.hpp written out against parq_amd/f1_eval.py iou3d: 1e-12 (the bound of test_gpu_eval_iou.py), zero where it is zero."""
    boxes = E.random_boxes(40, 5)
    worst, positive = 0.0, 0
    for i in range(40):
        for j in range(40):
            want = float(f1_eval.iou3d(boxes[i], boxes[j])[0])
            got = F.pair_iou_statement(boxes[i], boxes[j])
            assert (got == 0.0) == (want == 0.0), (i, j)
            worst = max(worst, abs(got - want))
            positive += want > 0
    print("max |statement - host| = %.3e over %d overlapping pairs" % (worst, positive))
    assert worst <= 1e-12 and positive > 200
    assert F.device_iou(np.full((8, 3), np.inf, np.float32), boxes[1].astype(np.float32)) == 0.0


# ---- the counts statement against count_matches ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["g12", "duplicate"])
def test_counts_statement_equals_count_matches_on_the_evaluator_runs(case):
    calc = _host_hash_run(F.g12_steps() if case == "g12" else F.duplicate_steps(), 0)
    names = list(calc.preds)
    counts, invalid, best = F.counts_statement([F.entries_store(calc.preds[n], 64) for n in names], [F.entries_store(calc.gts[n], 64) for n in names])
    assert np.array_equal(counts, F.host_counts(calc)) and not invalid.any()
    assert counts[0].sum() == sum(len(v) for v in calc.gts.values()) and counts[2].sum() > 0
    metrics = calc.compute_metrics()
    for t, thr in enumerate(F.THRESHOLDS):
        acc, rec, f1 = f1_eval.f1_from_counts(counts[0].tolist(), counts[1].tolist(), counts[2 + t].tolist())
        assert (metrics["%s_accuracy" % thr], metrics["%s_recall" % thr], metrics["%s_f1" % thr]) == (acc, rec, f1)


@pytest.mark.parametrize("seed", [0, 1])
def test_counts_statement_equals_count_matches_on_random_stores(seed):
    rng = np.random.RandomState(100 + seed)
    calc = F1Calculator(0.1)
    preds, gts = [], []
    for s in range(4):
        g = F.random_store(int(rng.randint(0, 14)), 16, 10 * seed + s)
        p = F.random_store(int(rng.randint(0, 20)), 24, 50 + 10 * seed + s, around=g)
        gts.append(g)
        preds.append(p)
        calc.gts["s%d" % s] = [(int(g["labels"][t]), g["corners"][t], 1) for t in range(g["count"])]
        calc.preds["s%d" % s] = [[int(p["labels"][t]), p["corners"][t], p["scores"][t], t] for t in range(p["count"])]
    counts, invalid, best = F.counts_statement(preds, gts)
    assert np.array_equal(counts, F.host_counts(calc)) and not invalid.any()
    assert counts[2].sum() > counts[4].sum() > 0                       # the thresholds separate


def test_counts_case_holds_what_its_docstring_says():
    preds, gts, mt_p, mt_g = F.counts_case()
    counts, invalid, best = F.counts_statement(preds, gts)
    assert sorted({s["count"] for s in preds}) == [0, 1, 65] and sorted({s["count"] for s in gts}) == [0, 1, 65]
    assert counts[0, 7] == 0 and counts[1, 7] > 0 and counts[0, 8] > 0 and counts[1, 8] == 0 and not counts[2:, 7:].any()
    assert invalid.tolist() == [1, 0]
    assert counts[2].sum() > counts[3].sum() > counts[4].sum() > 0


# ---- header, binding, exports ------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_binding_types_them():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    for name, names in NEW.items():
        m = re.search(r"\b(?:int|size_t)\s+\(%s\)\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/parq_hip.h must declare %s with a parenthesised name" % name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names, name
        assert name in _lib.EVAL_SYMBOLS and not any(name in t for t in _lib.ALL_TABLES)
        res, args = _lib.EVAL_SYMBOLS[name]
        assert len(args) == len(names) and res is (C.c_size_t if name.endswith("bytes") else C.c_int)
    assert len(_lib.EVAL_SYMBOLS) == 4 and _lib.EVAL_SYMBOLS not in _lib.ALL_TABLES
    assert sum(len(t) for t in _lib.ALL_TABLES) == 92
    assert "96" in open(os.path.join(ROOT, "README.md")).read()
    from parq_amd import scene_tracks
    assert parq_amd.f1_counts is f1_counts is scene_tracks.f1_counts and callable(SceneTracks.update_labelled)
    from parq_amd.decoder import PARQDecoder
    assert PARQDecoder.gt_tracks_on_device is False


def test_library_exports_the_entry_points_and_sizes():
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EVAL_SYMBOLS[name][1] and fn.restype is _lib.EVAL_SYMBOLS[name][0]
    g, u = lib.parq_gt_tracks_update_workspace_bytes, lib.parq_tracks_update_workspace_bytes
    assert g(1, 70, 96) >= u(1, 70, 96) + 70 * 25 * 4 and g(1, 70, 96) % 16 == 0 and g(5, 70, 96) >= 5 * u(1, 70, 96) + 5 * 70 * 25 * 4
    assert g(1, 0, 8) == 0 and g(1, 2049, 8) == 0 and g(1, 8, 2049) == 0 and g(-1, 8, 8) == 0 and g(0, 8, 8) == 0
    f = lib.parq_f1_counts_workspace_bytes
    assert f(3, 40, 3, 9) >= (5 * 9 + 2) * 3 * 4 and f(3, 40, 3, 9) % 16 == 0 and f(6, 40, 3, 9) >= 2 * f(3, 40, 3, 9) - 16
    assert f(1, 0, 3, 9) == 0 and f(1, 2049, 3, 9) == 0 and f(1, 8, 0, 9) == 0 and f(1, 8, 9, 9) == 0 and f(1, 8, 3, 0) == 0 and f(-1, 8, 3, 9) == 0


def test_argument_errors_return_before_any_device_call():
    """PARQ_ERR_ARG (1) from checks made on the host: the pointers below are never dereferenced."""
    lib = _lib.load()
    p, odd = C.c_void_p(4096), C.c_void_p(4104)
    slots, visits = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(0, 3)
    need = lib.parq_gt_tracks_update_workspace_bytes(2, 8, 8)

    def u(store=p, S_cap=2, mt=8, sl=slots, vis=visits, B=2, c=p, lab=p, ok=p, P=8, ws=p, wsb=need):
        return lib.parq_gt_tracks_update(store, S_cap, mt, sl, vis, B, c, lab, ok, P, 0.1, 0, ws, wsb, None, None)
    assert u(B=0) == 0                                                        # no scene: valid, nothing launched
    for bad in (dict(P=0), dict(P=2049), dict(mt=0), dict(mt=2049), dict(B=-1), dict(S_cap=-1), dict(store=None), dict(sl=None),
                dict(vis=None), dict(c=None), dict(lab=None), dict(ok=None), dict(ws=None), dict(wsb=need - 1), dict(ws=odd), dict(S_cap=1),
                dict(sl=(C.c_int32 * 2)(1, 1)), dict(sl=(C.c_int32 * 2)(0, -1)), dict(vis=(C.c_int32 * 2)(0, -1))):
        assert u(**bad) == 1, bad
    assert b"parq_gt_tracks_update" in lib.parq_last_error()
    thr = (C.c_double * 3)(0.25, 0.5, 0.7)
    need = lib.parq_f1_counts_workspace_bytes(2, 8, 3, 9)

    def f(ps=p, pm=8, gs=p, gm=8, S=2, th=thr, T=3, K=9, ws=p, wsb=need, counts=p, invalid=p):
        return lib.parq_f1_counts(ps, pm, gs, gm, S, th, T, K, ws, wsb, counts, invalid, None, None)
    for bad in (dict(S=-1), dict(S=65536), dict(pm=0), dict(pm=2049), dict(gm=0), dict(gm=2049), dict(T=0), dict(T=9), dict(K=0), dict(K=33),
                dict(ps=None), dict(gs=None), dict(th=None), dict(ws=None), dict(counts=None), dict(invalid=None), dict(wsb=need - 1),
                dict(ws=odd)):
        assert f(**bad) == 1, bad
    assert b"parq_f1_counts" in lib.parq_last_error()


def test_python_surface_checks_its_arguments_before_the_gpu():
    ok = dict(corners_world=torch.zeros(2, 5, 8, 3), labels=torch.zeros(2, 5, dtype=torch.int64), valid=torch.zeros(2, 5, dtype=torch.bool),
              n_names=2)
    assert check_labelled_args(**ok) == (2, 5)
    for key, bad, match in (("corners_world", torch.zeros(2, 5, 8, 2), "corners_world must be"),
                            ("corners_world", torch.zeros(2, 5, 8, 3, dtype=torch.int32), "corners_world must be"),
                            ("labels", torch.zeros(2, 5), "labels must be"), ("labels", torch.zeros(2, 4, dtype=torch.int32), "labels must be"),
                            ("valid", torch.zeros(2, 5), "valid must be"), ("n_names", 3, "scene names")):
        a = dict(ok)
        a[key] = bad
        with pytest.raises(ValueError, match=match):
            check_labelled_args(**a)
    with pytest.raises(ValueError, match="P = 2049"):
        check_labelled_args(torch.zeros(1, 2049, 8, 3), torch.zeros(1, 2049, dtype=torch.int32), torch.zeros(1, 2049, dtype=torch.bool), 1)
    with pytest.raises(ValueError, match="gt_jitter"):
        F1Calculator(0.1, gt_jitter="philox")
    with pytest.raises(ValueError, match="gt_store"):
        F1Calculator(0.1, gt_store="gpu")
    with pytest.raises(ValueError, match="track_store"):
        F1Calculator(0.1, gt_store="device")
    calc = F1Calculator(0.1, iou_device="cuda", track_store="device", gt_store="device", gt_seed=5)
    assert (calc.gt_jitter, calc.gt_seed, calc.on_device_gt) == ("hash", 5, True)
    with pytest.raises(TypeError):
        f1_counts(None, None, [0.5])
