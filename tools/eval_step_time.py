"""Cost of a validation step and of the end-of-epoch metrics with the ground-truth tracks and the F1 counts on the device
(PARQDecoder.gt_tracks_on_device; include/parq_hip.h parq_gt_tracks_update, parq_f1_counts) against the same path with the flag off:
metrics_on_device and tracks_on_device on, the ground-truth store on the host — the parent's behaviour, in the same process.

    python tools/eval_step_time.py [--repeats 5] [--out profiles/eval_on_device.json]

Two workloads, the two settings alternating, the first repeat dropped as warm-up:
  step      PARQDecoder.update_metrics ending in torch.cuda.synchronize(): 4 scenes, about 30 detections per scene against about 80
            prediction tracks, 12 ground-truth boxes per scene against 40 ground-truth tracks (the actual numbers are recorded);
            every repeat starts from the same stores.
  metrics   F1Calculator.compute_metrics: 100 scenes x 100 prediction tracks x 40 ground-truth tracks.
Reported: every repeat, the medians, the repeat spread (the largest max - min of either setting).  A gain is claimed only where the
difference of the medians exceeds the spread; otherwise the record says "no gain claimed"."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP = dict(scenes=4, queries=64, dets=30, world=80, gt_boxes=12, gt_world=40, seed=12)
METRICS = dict(scenes=100, tracks=100, gt_tracks=40, seed=13)


def step_world(w):
    """Per scene `world` upright boxes on a 3 m grid: (centre, full size, yaw, class)."""
    rng = np.random.RandomState(w["seed"])
    return [[(np.array([3.0 * (k % 9), 3.0 * (k // 9), 0.5]), rng.uniform(0.5, 1.2, 3), rng.uniform(-np.pi, np.pi), int(rng.randint(0, 9)))
             for k in range(w["world"])] for _ in range(w["scenes"])]


def decoder_outputs(world, first, w, rng, K):
    """Last-iteration outputs that show boxes [first, first + dets) of every scene on the leading queries, background elsewhere."""
    import torch
    B, Q = w["scenes"], w["queries"]
    center = rng.uniform(-90, -50, (B, Q, 3)).astype(np.float32)
    size = rng.uniform(0.4, 1.2, (B, Q, 3)).astype(np.float32)
    rot6 = np.zeros((B, Q, 6), np.float32)
    rot6[..., 0] = rot6[..., 5] = 1.0
    prob = np.full((B, Q, K), 0.01, np.float32)
    prob[..., K - 1] = 1.0 - 0.01 * (K - 1)
    for b in range(B):
        for q in range(w["dets"]):
            cen, full, yaw, cls = world[b][(first + q) % w["world"]]
            center[b, q] = cen + rng.normal(0, 0.02, 3)
            size[b, q] = full
            rot6[b, q] = (np.cos(yaw), np.sin(yaw), 0.0, 0.0, 0.0, 1.0)
            prob[b, q] = 0.01
            prob[b, q, cls] = 1.0 - 0.01 * (K - 1)
    to = lambda a: torch.from_numpy(a).cuda()
    return [{"center_unnormalized": to(center), "size_unnormalized": to(size), "ortho6d": to(rot6), "sem_cls_prob": to(prob)}]


def gt_padded(world, first, w, max_box=16):
    """obbs_padded (B, max_box, 19): ground-truth boxes [first, first + gt_boxes) of the first gt_world boxes of every scene, upright
    (object y along world z), rows beyond them -1."""
    import torch
    B = w["scenes"]
    X = -np.ones((B, max_box, 19), np.float32)
    up = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    for b in range(B):
        for j in range(w["gt_boxes"]):
            cen, full, yaw, cls = world[b][(first + j) % w["gt_world"]]
            c, s = np.cos(yaw), np.sin(yaw)
            R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ up
            h = full / 2
            X[b, j] = np.concatenate([[-h[0], h[0], -h[1], h[1], -h[2], h[2]], R.reshape(-1), cen, [cls]])
    return torch.from_numpy(X).cuda()


def snapshot(calc):
    s = dict(pred=calc._tracks._store.clone(), gts=copy.deepcopy(calc.gts), slots=dict(calc._gt_slots), visits=dict(calc._gt_visits))
    if calc._gt_tracks is not None:
        s.update(gt=calc._gt_tracks._store.clone(), gt_visits=dict(calc._gt_tracks._visits))
    return s


def restore(calc, s):
    calc._tracks._store.copy_(s["pred"])
    calc.gts, calc._gt_slots, calc._gt_visits = copy.deepcopy(s["gts"]), dict(s["slots"]), dict(s["visits"])
    if "gt" in s:
        calc._gt_tracks._store.copy_(s["gt"])
        calc._gt_tracks._visits = dict(s["gt_visits"])


def summarise(times, what, repeats):
    times = {k: v[1:] for k, v in times.items()}                      # the first repeat warms up
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = max(max(v) - min(v) for v in times.values())
    gain = med["flag_off"] - med["flag_on"]
    return {"what": "%s, the two settings alternating, %d repeats after one warm-up" % (what, repeats), "ms": times, "median_ms": med,
            "repeat_spread_ms": spread, "off_minus_on_ms": gain,
            "claim": ("gain of %.3f ms per call (above the repeat spread of %.3f ms)" % (gain, spread)) if gain > spread
            else "no gain claimed (difference %.3f ms, repeat spread %.3f ms)" % (gain, spread)}


def step_workload(repeats):
    import torch
    from parq_amd import Obb3D, Pose, synth
    from parq_amd.decoder import PARQDecoder
    w = STEP
    world = step_world(w)
    T_wl = Pose(torch.tensor([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).repeat(w["scenes"], 1, 1).cuda())
    names = ["scene%d" % s for s in range(w["scenes"])]
    decs, saved = {}, {}
    for key, on in (("flag_off", False), ("flag_on", True)):
        cfg = synth.decoder_cfg(dim=64, queries=w["queries"], heads=1, ffn=64, layers=1)
        cfg.TRACK_SCALE = [-100.0, 100.0] * 3
        dec = PARQDecoder(cfg).cuda().eval()
        dec.metrics_on_device = dec.tracks_on_device = True
        dec.gt_tracks_on_device = on
        rng = np.random.RandomState(w["seed"] + 1)
        np.random.seed(w["seed"])
        for first_pred, first_gt in ((0, 0), (25, 12), (50, 24), (55, 28)):          # fill the stores: 80 boxes seen, 40 ground-truth boxes
            dec.update_metrics(decoder_outputs(world, first_pred, w, rng, dec.num_semcls + 1), Obb3D(gt_padded(world, first_gt, w)), T_wl, names)
        decs[key], saved[key] = dec, snapshot(dec.metrics_calculator[0])
    rng = np.random.RandomState(w["seed"] + 2)
    outs, gt = decoder_outputs(world, 20, w, rng, decs["flag_on"].num_semcls + 1), Obb3D(gt_padded(world, 6, w))
    times = {"flag_off": [], "flag_on": []}
    for _ in range(repeats + 1):
        for key, dec in decs.items():
            restore(dec.metrics_calculator[0], saved[key])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.update_metrics([dict(outs[0])], gt, T_wl, names)
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e3)
    shape = {}
    for key, dec in decs.items():
        calc = dec.metrics_calculator[0]
        restore(calc, saved[key])
        calc.pull_tracks()
        shape[key] = {"prediction_tracks_before": [len(calc.preds[n]) for n in names], "gt_tracks_before": [len(calc.gts[n]) for n in names]}
    det = decs["flag_on"].parse_pred([dict(outs[0])])
    shape["detections"] = ((det["sem_cls_prob"].argmax(-1) != decs["flag_on"].num_semcls) & det["pred_mask"]).sum(-1).tolist()
    row = summarise(times, "host wall time of PARQDecoder.update_metrics ending in torch.cuda.synchronize()", repeats)
    row["workload"] = dict(w, **shape)
    return row


def metrics_workload(repeats):
    import torch
    from eval_iou_ab import yaw_box
    from parq_amd.f1_eval import F1Calculator
    w = METRICS
    rng = np.random.RandomState(w["seed"])
    S, n, g = w["scenes"], w["tracks"], w["gt_tracks"]
    corners = np.zeros((S, n, 8, 3), np.float32)
    gt_corners = np.zeros((S, g, 8, 3), np.float32)
    prob = np.full((S, n, 10), 0.02, np.float32)
    labels = rng.randint(0, 9, (S, g))
    for s in range(S):
        for k in range(n):
            cen, half, yaw = np.array([3.0 * (k % 10), 3.0 * (k // 10), 0.5]), rng.uniform(0.25, 0.6, 3), rng.uniform(-np.pi, np.pi)
            corners[s, k] = yaw_box(cen + rng.normal(0, 0.05, 3), half, yaw)
            prob[s, k, labels[s, k] if k < g and rng.rand() < 0.8 else rng.randint(0, 9)] = 0.8
            if k < g:
                gt_corners[s, k] = yaw_box(cen, half * rng.uniform(0.9, 1.1, 3), yaw)
    dev = lambda a: torch.from_numpy(a).cuda()
    out = {"pred_corners_world": dev(corners), "sem_cls_prob": dev(prob), "pred_mask": dev(np.ones((S, n), bool)),
           "scene_name": ["scene%d" % s for s in range(S)]}
    gts = [{"labels": dev(labels[s]), "gt_corners_world": dev(gt_corners[s])} for s in range(S)]
    calcs = {"flag_off": F1Calculator(0.1, iou_device="cuda", track_store="device"),
             "flag_on": F1Calculator(0.1, iou_device="cuda", track_store="device", gt_store="device")}
    np.random.seed(w["seed"])
    for calc in calcs.values():
        calc.step(out, gts)
    times, metrics = {"flag_off": [], "flag_on": []}, {}
    for _ in range(repeats + 1):
        for key, calc in calcs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            metrics[key] = calc.compute_metrics()
            times[key].append((time.perf_counter() - t0) * 1e3)
    row = summarise(times, "host wall time of F1Calculator.compute_metrics (it ends with its results on the host)", repeats)
    calcs["flag_on"].pull_tracks()
    row["workload"] = dict(w, prediction_tracks=sorted({len(t) for t in calcs["flag_on"].preds.values()}),
                           gt_tracks=sorted({len(t) for t in calcs["flag_on"].gts.values()}))
    row["metrics"] = metrics                                          # different jitter sources: close, not necessarily equal
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rec = {"box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName},
           "baseline": "metrics_on_device and tracks_on_device on, gt_tracks_on_device off: the ground-truth store on the host, as before this flag",
           "step": step_workload(a.repeats)}
    print(json.dumps(rec["step"]), flush=True)
    rec["metrics"] = metrics_workload(a.repeats)
    print(json.dumps(rec["metrics"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
