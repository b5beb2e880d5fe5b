"""What average precision adds to the end-of-epoch metrics (F1Calculator average_precision; include/parq_hip.h parq_average_precision)
over the same calculator with the flag off, which is the parent's compute_metrics: both stores on the device, one parq_f1_counts
call and one small copy.

    python tools/average_precision_time.py [--repeats 5] [--out profiles/average_precision.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/average_precision_time.py --trace-calls 20 [--shape epoch]

Two workloads:
  eval    100 scenes x 100 prediction tracks x 40 ground-truth tracks: the shape of profiles/eval_on_device.json.
  epoch   300 scenes x 150 prediction tracks x 40 ground-truth tracks in stores of capacity 512: near a ScanNet validation epoch
          (153600 store positions, sorted as 262144 keys).
Measured: host wall time of F1Calculator.compute_metrics, which ends with its results on the host, the flag off and on alternating
in one process, the first repeat dropped as warm-up.  Reported: every repeat, the medians, the repeat spread (the largest max - min
of either setting).  A cost is claimed only where the difference of the medians exceeds the spread; otherwise the record says "no
cost claimed".  The host statement (f1_eval.average_precision_host over the pulled track lists) is timed once: with the IoU
matrices taken from one parq_obb_iou launch, as the calculator's host path with iou_device does, and on `eval` also pair by pair
on the host, as with iou_device=None.  --trace-calls N runs N flag-on calls and nothing else, for a profiler run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"eval": dict(scenes=100, tracks=100, gt_tracks=40, capacity=2048, seed=13),
          "epoch": dict(scenes=300, tracks=150, gt_tracks=40, capacity=512, seed=14)}
THRESHOLDS = (0.25, 0.5)


def build(w):
    """A calculator with both stores on the device, fed one batch: per scene `tracks` boxes on a 3 m grid, each its own track, the
    first `gt_tracks` of them noisy copies of a ground-truth box (80 % with its label); scores spread over (0.15, 0.95)."""
    import torch
    from eval_iou_ab import yaw_box
    from parq_amd.f1_eval import F1Calculator
    rng = np.random.RandomState(w["seed"])
    S, n, g = w["scenes"], w["tracks"], w["gt_tracks"]
    corners = np.zeros((S, n, 8, 3), np.float32)
    gt_corners = np.zeros((S, g, 8, 3), np.float32)
    prob = np.zeros((S, n, 10), np.float32)
    labels = rng.randint(0, 9, (S, g))
    for s in range(S):
        for k in range(n):
            cen, half, yaw = np.array([3.0 * (k % 13), 3.0 * (k // 13), 0.5]), rng.uniform(0.25, 0.6, 3), rng.uniform(-np.pi, np.pi)
            corners[s, k] = yaw_box(cen + rng.normal(0, 0.08, 3), half, yaw)
            top = rng.uniform(0.15, 0.95)
            prob[s, k] = (1.0 - top) / 9.0
            prob[s, k, labels[s, k] if k < g and rng.rand() < 0.8 else rng.randint(0, 9)] = top
            if k < g:
                gt_corners[s, k] = yaw_box(cen, half * rng.uniform(0.9, 1.1, 3), yaw)
    dev = lambda a: torch.from_numpy(a).cuda()
    out = {"pred_corners_world": dev(corners), "sem_cls_prob": dev(prob), "pred_mask": dev(np.ones((S, n), bool)),
           "scene_name": ["scene%d" % s for s in range(S)]}
    gts = [{"labels": dev(labels[s]), "gt_corners_world": dev(gt_corners[s])} for s in range(S)]
    calc = F1Calculator(0.1, f1_iou_thresh=THRESHOLDS, iou_device="cuda", track_store="device", gt_store="device")
    calc.track_capacity = w["capacity"]
    calc.step(out, gts)
    return calc


def summarise(times, repeats):
    times = {k: v[1:] for k, v in times.items()}                      # the first repeat warms up
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(max(v) - min(v) for v in times.values())
    cost = med["flag_on"] - med["flag_off"]
    return {"what": "host wall time of F1Calculator.compute_metrics (it ends with its results on the host), the flag off and on "
                    "alternating, %d repeats after one warm-up" % repeats,
            "ms": times, "median_ms": med, "repeat_spread_ms": spread, "on_minus_off_ms": cost,
            "claim": ("cost of %.3f ms per call (above the repeat spread of %.3f ms)" % (cost, spread)) if cost > spread
            else "no cost claimed (difference %.3f ms, repeat spread %.3f ms)" % (cost, spread)}


def workload(name, repeats):
    import torch
    from parq_amd.f1_eval import CARE_CLASSES, DeviceIoU, average_precision_host, canonical_stack
    w = SHAPES[name]
    calc = build(w)
    times, metrics = {"flag_off": [], "flag_on": []}, {}
    for _ in range(repeats + 1):
        for key, on in (("flag_off", False), ("flag_on", True)):
            calc.average_precision = on
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            metrics[key] = calc.compute_metrics()
            times[key].append((time.perf_counter() - t0) * 1e3)
    row = summarise(times, repeats)
    assert {k: v for k, v in metrics["flag_on"].items() if k in metrics["flag_off"]} == metrics["flag_off"]
    calc.pull_tracks()
    names = list(calc.preds)
    preds, gts = [calc.preds[s] for s in names], [calc.gts[s] for s in names]
    host = {}
    t0 = time.perf_counter()
    ious = DeviceIoU("cuda")([(canonical_stack(g), canonical_stack(p)) for g, p in zip(gts, preds)])
    res = average_precision_host(preds, gts, THRESHOLDS, len(CARE_CLASSES), ious=ious)
    host["iou_matrices_from_one_parq_obb_iou_launch_ms"] = (time.perf_counter() - t0) * 1e3
    same = all(float(res["ap"][t][c]) == metrics["flag_on"]["%s_AP_%s" % (thr, cname)]
               for t, thr in enumerate(THRESHOLDS) for c, cname in CARE_CLASSES.items())
    if name == "eval":
        t0 = time.perf_counter()
        average_precision_host(preds, gts, THRESHOLDS, len(CARE_CLASSES))
        host["pair_by_pair_on_the_host_ms"] = (time.perf_counter() - t0) * 1e3
    row["host_statement_once"] = dict(host, equals_the_device_values=bool(same),
                                      what="f1_eval.average_precision_host over the pulled track lists, timed once, the pull not included")
    cs = res["class_start"]
    last = [int(cs[c + 1]) - 1 for c in range(len(CARE_CLASSES)) if cs[c + 1] > cs[c]]         # the last rank of every class that has one
    row["workload"] = dict(w, thresholds=list(THRESHOLDS), prediction_tracks=sorted({len(t) for t in preds}),
                           gt_tracks=sorted({len(t) for t in gts}), ranked=int(cs[-1]),
                           true_positives=[int(sum(res["cum_tp"][t][r] for r in last)) for t in range(len(THRESHOLDS))])
    row["metrics"] = {k: v for k, v in metrics["flag_on"].items() if "mAP" in k or "f1" in k}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--shape", default="epoch", choices=sorted(SHAPES))
    a = ap.parse_args()
    import torch
    if a.trace_calls:
        calc = build(SHAPES[a.shape])
        calc.average_precision = True
        for _ in range(a.trace_calls):
            calc.compute_metrics()
        torch.cuda.synchronize()
        return
    rec = {"box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName},
           "baseline": "the same calculator with average_precision off: the parent's compute_metrics (parq_f1_counts and one copy)",
           "note": "AP is not a number of the reference, whose evaluator has none; the oracle is the rule's statement"}
    for name in ("eval", "epoch"):
        rec[name] = workload(name, a.repeats)
        print(json.dumps(rec[name]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
