"""Cost of the evaluation tracker's oriented-box IoU on the host and on the device: F1Calculator.step on the same inputs with
iou_device=None and iou_device="cuda" (parq_amd/f1_eval.py, include/parq_hip.h parq_obb_iou).

    python tools/eval_iou_ab.py [--scenes 4] [--dets 30] [--tracks 80] [--repeats 5] [--out profiles/eval_iou_ab.json]

Every scene holds `tracks` prediction tracks (seeded yaw boxes in a room) when the timed step arrives with `dets` detections per
scene, most of them noisy re-observations of a track, so the boxes overlap; the ground truth adds a few pairs per scene.  The timed
call is the whole step (parse, canonical corners, IoU, assignment, track update) from the same tracker state each time; the device
path's IoU call (pack, upload, launch, copy back) is timed inside it.  Both paths must leave the same tracker state.  The record
also carries the kernel's register / scratch / LDS figures, read from the assembly hipcc writes for csrc/obb_iou.hip."""
import argparse
import copy
import json
import os
import platform
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def yaw_box(center, half, yaw):
    """World corners (8,3), Obb3D.bb3corners_object order, object y along world +z (what the IoU routine assumes)."""
    sx, sy, sz = half
    obj = np.array([[-sx, -sy, -sz], [sx, -sy, -sz], [sx, sy, -sz], [-sx, sy, -sz], [-sx, -sy, sz], [sx, -sy, sz], [sx, sy, sz], [-sx, sy, sz]])
    c, s = np.cos(yaw), np.sin(yaw)
    return obj @ (np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])).T + center


def make_inputs(rng, scenes, tracks, dets, ngt=10):
    def probs(n):
        p = np.full((n, 10), 0.02, np.float32)
        p[np.arange(n), rng.randint(0, 9, n)] = rng.uniform(0.4, 0.8, n)
        return p
    world = [[(rng.uniform(-3, 3, 3) * np.array([1, 1, 0.3]), rng.uniform(0.125, 0.75, 3), rng.uniform(-np.pi, np.pi)) for _ in range(tracks)]
             for _ in range(scenes)]
    names = ["scene%d" % s for s in range(scenes)]
    first = {"pred_corners_world": np.stack([np.stack([yaw_box(*b) for b in w]) for w in world]).astype(np.float32),
             "sem_cls_prob": np.stack([probs(tracks) for _ in world]), "pred_mask": np.ones((scenes, tracks), bool), "scene_name": names}
    seen = []
    for w in world:
        boxes = []
        for k in range(dets):
            if k < dets * 3 // 4:                                    # a re-observation of track k, jittered
                cen, half, yaw = w[k % tracks]
                boxes.append(yaw_box(cen + rng.normal(0, 0.08, 3), half * rng.uniform(0.85, 1.15, 3), yaw + rng.normal(0, 0.1)))
            else:                                                    # something new
                boxes.append(yaw_box(rng.uniform(-3, 3, 3) * np.array([1, 1, 0.3]), rng.uniform(0.125, 0.75, 3), rng.uniform(-np.pi, np.pi)))
        seen.append(np.stack(boxes))
    second = {"pred_corners_world": np.stack(seen).astype(np.float32), "sem_cls_prob": np.stack([probs(dets) for _ in world]),
              "pred_mask": np.ones((scenes, dets), bool), "scene_name": names}
    gts = [{"labels": rng.randint(0, 9, ngt), "gt_corners_world": first["pred_corners_world"][s, :ngt]} for s in range(scenes)]
    return first, second, gts


def kernel_stats():
    """{"vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"} of obb_iou_kernel, or None without hipcc."""
    src = os.path.join(ROOT, "parq_amd", "csrc", "obb_iou.hip")
    hipcc = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
    try:
        asm = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", "-", src],
                             capture_output=True, text=True, timeout=300, check=True).stdout
    except (OSError, subprocess.SubprocessError):
        return None
    block = asm[asm.index("amdhsa.kernels"):]
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
            for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}


def state(calc):
    return {n: [(int(t[0]), np.asarray(t[1]).tolist(), float(t[2]), int(t[3])) for t in trks] for n, trks in calc.preds.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--dets", type=int, default=30)
    ap.add_argument("--tracks", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from parq_amd.f1_eval import F1Calculator
    first, second, gts = make_inputs(np.random.RandomState(a.seed), a.scenes, a.tracks, a.dets)
    times, iou_call, final, pairs = {}, [], {}, None
    for name, device in (("host", None), ("device", "cuda")):
        calc = F1Calculator(0.1, iou_device=device)
        np.random.seed(a.seed)
        calc.step(first, gts)
        assert all(len(t) == a.tracks for t in calc.preds.values())
        if device is not None:
            backend = calc.iou_backend

            def timed(segments, _inner=backend):
                t0 = time.perf_counter()
                out = _inner(segments)
                iou_call.append((time.perf_counter() - t0) * 1e3)
                return out
            calc.iou_backend = timed
        saved = (copy.deepcopy(calc.preds), copy.deepcopy(calc.gts))
        rows = []
        for rep in range(a.repeats + 1):                             # the first repeat warms up (library load, allocator) and is dropped
            calc.preds, calc.gts = copy.deepcopy(saved[0]), copy.deepcopy(saved[1])
            np.random.seed(a.seed + 1)
            t0 = time.perf_counter()
            calc.step(second, gts)
            rows.append((time.perf_counter() - t0) * 1e3)
        times[name] = rows[1:]
        final[name] = state(calc)
        if device is not None:
            pairs = backend.pairs // backend.launches
            assert backend.launches == a.repeats + 1, backend.launches
        print("%-6s step: %s ms" % (name, ", ".join("%.2f" % r for r in rows[1:])), flush=True)
    assert final["host"] == final["device"], "host and device paths left different tracks"
    med = {k: statistics.median(v) for k, v in times.items()}
    call = statistics.median(iou_call[1:])
    ratio = med["host"] / med["device"]
    cpu = [ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")][:1] if os.path.exists("/proc/cpuinfo") else []
    rec = {"workload": "F1Calculator.step, %d scenes x (%d detections x %d tracks) + ground truth, one batch" % (a.scenes, a.dets, a.tracks),
           "pairs_per_step": pairs, "host_ms": times["host"], "device_ms": times["device"], "host_ms_median": med["host"],
           "device_ms_median": med["device"], "host_over_device": ratio,
           "device_iou_call_ms_median": call, "device_rest_ms_median": med["device"] - call,
           "host_us_per_pair": med["host"] * 1e3 / pairs,
           "box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName, "host_cpu": cpu[0] if cpu else platform.processor()},
           "kernel": kernel_stats(),
           "note": "device_iou_call = pack + one upload + one launch + one copy back; device_rest = parse, canonical corners, float32 cast, "
                   "LSAP, track update and deep copies, which both paths share."}
    if ratio < 5:
        rec["note"] += "  Ratio under 5x: the device path is bounded by device_rest (host bookkeeping), not by the IoU call."
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
