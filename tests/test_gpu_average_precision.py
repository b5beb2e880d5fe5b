"""GPU tier of the average precision: parq_average_precision (csrc/avg_precision.hip) against its NumPy statement
(tests/average_precision_cases.py) exactly, every output, then parq_amd.average_precision, F1Calculator(average_precision=True) with
both stores on the device and PARQDecoder.average_precision against the host calculator in "hash" mode.  The reference's evaluator
has no AP: the statement and its sequential twin (test_average_precision_cpu.py) are the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import average_precision_cases as A
import eval_iou_cases as E
import f1_device_cases as F
import parq_amd
from gpu_util import lib
from oracle.make_golden import F1_CASE
from parq_amd import Obb3D, Pose, SceneTracks, _lib
from parq_amd.f1_eval import CARE_CLASSES, F1Calculator

pytestmark = pytest.mark.gpu

CANARY = -77
GUARD = 4


def vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def run_raw(preds, gts, mt_p, mt_g, thresholds, K=A.K_CARE, curves=True, pred_words=None, gt_words=None):
    """One call of the raw entry on statement stores; every output has a guard behind it.  Returns the outputs as NumPy arrays."""
    l = lib()
    S, T = len(preds), len(thresholds)
    N = S * mt_p
    ps = torch.from_numpy(A.store_words(preds, mt_p) if pred_words is None else pred_words).cuda()
    gs = torch.from_numpy(A.store_words(gts, mt_g) if gt_words is None else gt_words).cuda()
    need = l.parq_average_precision_workspace_bytes(S, mt_p, mt_g, T, K)
    assert need > 0 and need % 16 == 0
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    n = (T + 2) * K + 2
    out = torch.full((n + GUARD,), CANARY, dtype=torch.int64, device="cuda")
    opt = None
    if curves:
        opt = dict(order=torch.full((N + GUARD,), CANARY, dtype=torch.int32, device="cuda"),
                   class_start=torch.full((K + 1 + GUARD,), CANARY, dtype=torch.int32, device="cuda"),
                   cum_tp=torch.full((T * N + GUARD,), CANARY, dtype=torch.int32, device="cuda"),
                   pred_best=torch.full((N + GUARD,), -7.0, dtype=torch.float64, device="cuda"),
                   pred_target=torch.full((N + GUARD,), CANARY, dtype=torch.int32, device="cuda"))
    ptrs = [vp(opt[k]) if curves else None for k in ("order", "class_start", "cum_tp", "pred_best", "pred_target")]
    rc = l.parq_average_precision(vp(ps), mt_p, vp(gs), mt_g, S, (C.c_double * T)(*thresholds), T, K, vp(ws), need, vp(out), vp(out[T * K:]),
                                  vp(out[(T + 2) * K:]), *ptrs, _lib.stream_ptr())
    assert rc == 0, l.parq_last_error()
    host = out.cpu().numpy()
    assert (host[n:] == CANARY).all() and bool((ws[need:] == 0x5A).all())
    got = dict(ap=host[:T * K].view(np.float64).reshape(T, K), counts=host[T * K:(T + 2) * K].reshape(2, K), invalid=host[(T + 2) * K:n])
    if curves:
        o = {k: v.cpu().numpy() for k, v in opt.items()}
        assert (o["order"][N:] == CANARY).all() and (o["class_start"][K + 1:] == CANARY).all() and (o["cum_tp"][T * N:] == CANARY).all()
        assert (o["pred_best"][N:] == -7.0).all() and (o["pred_target"][N:] == CANARY).all()
        got.update(order=o["order"][:N], class_start=o["class_start"][:K + 1], cum_tp=o["cum_tp"][:T * N].reshape(T, N),
                   pred_best=o["pred_best"][:N].reshape(S, mt_p), pred_target=o["pred_target"][:N].reshape(S, mt_p))
    return got


def assert_equals_statement(got, want, what=""):
    """Every output equal exactly: integers as integers, float64 by their bits."""
    assert np.array_equal(got["counts"], want["counts"]), (what, got["counts"], want["counts"])
    assert got["invalid"].tolist() == want["invalid"].tolist(), what
    if "order" in got:
        assert np.array_equal(got["class_start"], want["class_start"]), (what, got["class_start"], want["class_start"])
        assert np.array_equal(got["order"], want["order"]), what
        assert np.array_equal(got["cum_tp"], want["cum_tp"]), what
        for s, (b, tg) in enumerate(zip(want["pred_best"], want["pred_target"])):
            k = len(b)
            assert np.array_equal(got["pred_target"][s, :k], tg), (what, s)
            assert np.array_equal(got["pred_best"][s, :k].view(np.int64), b.view(np.int64)), (what, s)
            assert (got["pred_best"][s, k:] == -7.0).all() and (got["pred_target"][s, k:] == CANARY).all(), (what, s)   # not written
    assert np.array_equal(got["ap"].view(np.int64), want["ap"].view(np.int64)), (what, got["ap"], want["ap"])


def test_raw_entry_equals_the_statement_and_two_calls_give_the_same_bits():
    """f1_device_cases.counts_case() with random scores: 0, 1 and 65 tracks per side (past one wavefront), an out-of-range label,
    classes with one side only.  Every output, the optional ones included; without them the same three."""
    preds, gts, mt_p, mt_g = A.scored_counts_case()
    thresholds = (0.25, 0.5, 0.7)
    want = A.ap_statement(preds, gts, thresholds)
    assert want["pairs"] < 2000 and want["invalid"].tolist() == [1, 0] and want["flags"].sum() > 20
    first = run_raw(preds, gts, mt_p, mt_g, thresholds)
    assert_equals_statement(first, want)
    again = run_raw(preds, gts, mt_p, mt_g, thresholds)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k
    plain = run_raw(preds, gts, mt_p, mt_g, thresholds, curves=False)
    assert_equals_statement(plain, want)
    assert 0 < want["ap"].max() <= 1.0


def test_hand_made_cases_on_the_device():
    preds, gts, expected = A.hand_case()
    want = A.ap_statement(preds, gts, A.HAND_THRESHOLDS)
    got = run_raw(preds, gts, A.HAND_MT_P, A.HAND_MT_G, A.HAND_THRESHOLDS)
    assert_equals_statement(got, want)
    assert np.array_equal(got["ap"], expected["ap"]) and got["invalid"].tolist() == expected["invalid"]
    n = len(expected["order"])
    assert [(int(o) // A.HAND_MT_P, int(o) % A.HAND_MT_P) for o in got["order"][:n]] == expected["order"] and (got["order"][n:] == -1).all()
    cs = got["class_start"]
    for t in range(3):
        marks = []                                                            # the steps of the cumulative counts, class by class
        for c in range(A.K_CARE):
            marks += np.diff(np.concatenate([[0], got["cum_tp"][t, cs[c]:cs[c + 1]]])).astype(bool).tolist()
        assert marks == [expected["flags"][sp][t] for sp in expected["order"]], t


def test_sort_case_across_tiles_equals_the_statement():
    """5400 positions padded to 8192, four tiles of 2048: classes 2 and 5 lie across ranks 2048 and 4096 of the sorted array."""
    preds, gts = A.sort_case()
    want = A.ap_statement(preds, gts, A.THRESHOLDS)
    cs = want["class_start"]
    assert want["pairs"] < 2000 and cs[2] < 2048 < cs[3] and cs[5] < 4096 < cs[6] and want["flags"].sum() >= 6
    got = run_raw(preds, gts, A.SORT_MT_P, A.SORT_MT_G, A.THRESHOLDS)
    assert_equals_statement(got, want)
    assert want["ap"][0, [0, 2, 5]].min() > 0 and want["invalid"][1] == 18


def test_capacity_one_on_both_sides():
    g = [A._fill(1, [(3, 0.0, 1)]), A._fill(1, []), A._fill(1, [(3, 0.0, 1)])]
    p = [A._fill(1, [(3, 0.1, 0.4)]), A._fill(1, [(3, 0.0, 0.9)]), A._fill(1, [(3, 0.7, 0.4)])]
    want = A.ap_statement(p, g, A.THRESHOLDS)
    assert want["order"].tolist() == [1, 0, 2] and want["flags"].tolist() == [[False, True, False]] * 2
    assert want["ap"][0, 3] == 0.5 / 2
    assert_equals_statement(run_raw(p, g, 1, 1, A.THRESHOLDS), want)
    one = ([A._fill(1, [(0, 0.1, 0.4)])], [A._fill(1, [(0, 0.0, 1)])])
    assert_equals_statement(run_raw(one[0], one[1], 1, 1, (0.5,), K=1), A.ap_statement(one[0], one[1], (0.5,), 1))


def test_a_corrupt_count_reads_as_an_empty_slot():
    preds, gts, mt_p, mt_g = A.scored_counts_case()
    pw, gw = A.store_words(preds, mt_p), A.store_words(gts, mt_g)
    assert preds[0]["count"] == 65 and gts[4]["count"] == 1 and preds[4]["count"] == 65
    pw[0, 0] = -1                                                             # slot 0's predictions, slot 4's ground truth
    gw[4, 0] = mt_g + 1
    bad_p = [dict(preds[0], count=-1)] + preds[1:]
    bad_g = gts[:4] + [dict(gts[4], count=mt_g + 1)] + gts[5:]
    want = A.ap_statement(bad_p, bad_g, A.THRESHOLDS)
    empty = A.ap_statement([F.T.empty_store(mt_p)] + preds[1:], gts[:4] + [F.T.empty_store(mt_g)] + gts[5:], A.THRESHOLDS)
    assert np.array_equal(want["ap"], empty["ap"]) and np.array_equal(want["order"], empty["order"])
    got = run_raw(preds, gts, mt_p, mt_g, A.THRESHOLDS, pred_words=pw, gt_words=gw)
    assert_equals_statement(got, want)
    assert (got["pred_target"][0] == CANARY).all()                            # nothing of the corrupt slot was written


def test_no_scene_zeroes_the_outputs():
    got = run_raw([], [], 8, 8, A.THRESHOLDS)
    assert not got["ap"].any() and not got["counts"].any() and not got["invalid"].any() and not got["class_start"].any()
    ap, counts, invalid = parq_amd.average_precision(SceneTracks(max_tracks=8), SceneTracks(max_tracks=8), A.THRESHOLDS)
    assert ap.shape == (2, 9) and ap.dtype == torch.float64 and counts.shape == (2, 9) and not ap.any() and not counts.any() and not invalid.any()


def _tracks_from(stores, mt):
    tracks = SceneTracks(max_tracks=mt, device="cuda:0")
    tracks._slots = {"scene%d" % s: s for s in range(len(stores))}
    tracks._store = torch.from_numpy(A.store_words(stores, mt)).cuda()
    return tracks


def test_the_python_call_equals_the_statement_and_only_enqueues():
    preds, gts, expected = A.hand_case()
    want = A.ap_statement(preds, gts, A.HAND_THRESHOLDS)
    pt, gt = _tracks_from(preds, A.HAND_MT_P), _tracks_from(gts, A.HAND_MT_G)
    parq_amd.average_precision(pt, gt, A.HAND_THRESHOLDS, curves=True)        # warm-up: the workspace, the library
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ap, counts, invalid, curve = parq_amd.average_precision(pt, gt, A.HAND_THRESHOLDS, curves=True)
        ap2, _, _ = parq_amd.average_precision(pt, gt, A.HAND_THRESHOLDS)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ap.is_cuda and ap.dtype == torch.float64 and tuple(ap.shape) == (3, 9) and counts.dtype == torch.int64
    assert np.array_equal(ap.cpu().numpy().view(np.int64), want["ap"].view(np.int64)) and torch.equal(ap, ap2)
    assert np.array_equal(counts.cpu().numpy(), want["counts"]) and invalid.tolist() == want["invalid"].tolist()
    assert np.array_equal(curve["order"].cpu().numpy(), want["order"]) and np.array_equal(curve["cum_tp"].cpu().numpy(), want["cum_tp"])
    assert np.array_equal(curve["class_start"].cpu().numpy(), want["class_start"])
    for s in range(2):
        k = preds[s]["count"]
        assert np.array_equal(curve["pred_target"][s, :k].cpu().numpy(), want["pred_target"][s])
        assert np.array_equal(curve["pred_best"][s, :k].cpu().numpy().view(np.int64), want["pred_best"][s].view(np.int64))


def _feed_device(calc, st):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = {"pred_corners_world": dev(st["corners"]), "sem_cls_prob": dev(st["prob"]), "pred_mask": dev(st["mask"]), "scene_name": st["scenes"]}
    calc.step(out, [{"labels": dev(x["labels"]), "gt_corners_world": dev(x["corners"])} for x in st["gts"]])


AP_KEYS = {"%s_%s" % (t, k) for t in (0.25, 0.5, 0.7) for k in ["mAP"] + ["AP_" + n for n in CARE_CLASSES.values()]}


def test_calculator_with_both_stores_on_the_device_returns_the_host_values_in_one_copy():
    steps, seed = F.g12_steps(), 5
    want = F.hash_calculator(seed, average_precision=True)
    for st in steps:
        E._feed(want, st)
    want_metrics = want.compute_metrics()
    nine = F.hash_calculator(seed)
    for st in steps:
        E._feed(nine, st)
    nine = nine.compute_metrics()
    assert len(nine) == 9 and {k: v for k, v in want_metrics.items() if k in nine} == nine and set(want_metrics) == set(nine) | AP_KEYS
    calc = F1Calculator(F1_CASE["conf"], iou_device="cuda", track_store="device", gt_store="device", gt_seed=seed, average_precision=True)
    for st in steps:
        _feed_device(calc, st)
    metrics = calc.compute_metrics()
    assert metrics == want_metrics, {k: (metrics[k], want_metrics[k]) for k in metrics if metrics[k] != want_metrics[k]}   # AP bit for bit
    assert max(metrics["%s_mAP" % t] for t in (0.25, 0.5, 0.7)) > 0
    assert (calc.count_launches, calc.count_copies, calc.ap_launches) == (1, 1, 1)
    assert calc.preds == {} and calc.gts == {}                                # nothing was pulled for the metrics
    calc.average_precision = False                                            # off: exactly the nine keys, nothing more launched
    assert calc.compute_metrics() == nine and calc.ap_launches == 1 and calc.count_copies == 2


def test_decoder_average_precision_on_top_of_the_three_device_flags():
    from parq_amd.decoder import PARQDecoder
    from test_gpu_f1_device import _tiny_decoder
    assert PARQDecoder.average_precision is False
    dec, outs, gt, T_wl, names = _tiny_decoder()
    dec.metrics_on_device = dec.tracks_on_device = True
    calc = dec.metrics_calculator[0]
    calc.gt_jitter, calc.gt_seed = "hash", 21
    results = {}
    for on in (False, True):                                                  # the host calculator in hash mode, then the device
        dec.gt_tracks_on_device = on
        dec.average_precision = True
        dec.reset_metrics()
        for _ in range(2):
            dec.update_metrics(outs, Obb3D(gt), Pose(T_wl), names)
        copies = calc.count_copies
        results[on] = dec.compute_metrics()
        assert calc.on_device_gt == on and calc.count_copies - copies == (1 if on else 0)
    assert results[True] == results[False] and set(results[True]) - AP_KEYS == {k for k in results[True] if "AP" not in k}
    assert len(results[True]) == 9 + len(AP_KEYS) and all(0.0 <= results[True][k] <= 1.0 for k in AP_KEYS)
    dec.average_precision = False
    assert set(dec.compute_metrics()) == {k for k in results[True] if "AP" not in k}
