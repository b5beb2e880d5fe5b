"""Cost of following detections across snippets on the device: SceneTracks.update (parq_amd/scene_tracks.py, include/parq_hip.h
parq_tracks_update) against the prediction side of F1Calculator(iou_device="cuda").step, the path it replaces.

    python tools/scene_tracks_time.py [--repeats 5] [--out profiles/scene_tracks.json] [--resources profiles/scene_tracks_kernel_resources.txt]

Two workloads: the one of tools/eval_iou_ab.py (4 scenes x 30 detections x 80 tracks, seed 12) and a larger one (8 scenes x 64
detections x 400 tracks).  Every scene holds its tracks when the timed step arrives; both paths start each repeat from that state,
read the same device tensors and must leave the same set of tracks.  Three kinds of numbers, each labelled for what it is:
  wall_ms     host wall time of one prediction-side step ending in a synchronise, the two paths alternating in one process;
  device_ms   device time of one update between two events on its stream;
  kernels     per-kernel times from separate `rocprofv3 --kernel-trace --stats` runs of this script with --kernels-only, one per workload.
The kernels' register / LDS / scratch figures, from the compiler's remarks for csrc/tracks.hip, go to --resources."""
import argparse
import copy
import csv
import glob
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

WORKLOADS = [dict(scenes=4, dets=30, tracks=80, seed=12), dict(scenes=8, dets=64, tracks=400, seed=12)]


def inputs(w):
    import torch
    from eval_iou_ab import make_inputs
    first, second, _ = make_inputs(np.random.RandomState(w["seed"]), w["scenes"], w["tracks"], w["dets"])
    dev = lambda d: {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    return dev(first), dev(second)


def feed(tracks, out):
    return tracks.update(out["scene_name"], out["pred_corners_world"], out["sem_cls_prob"], out["pred_mask"])


def sorted_tracks(entries):
    return sorted((int(e[0]), float(e[2]), np.ascontiguousarray(e[1], np.float32).tobytes()) for e in entries)


def kernels_only(k, repeats=20):
    """What a profiler run executes: the updates of workload k alone (the first call fills the store and is a first visit)."""
    import torch
    from parq_amd import SceneTracks
    first, second = inputs(WORKLOADS[k])
    tracks = SceneTracks(max_tracks=512)
    feed(tracks, first)
    saved = tracks._store.clone()
    for _ in range(repeats):
        tracks._store.copy_(saved)
        feed(tracks, second)
    torch.cuda.synchronize()


def profiler_kernels(k):
    """{kernel: {"calls", "avg_us"}} of the tracker's kernels from a child run of workload k under rocprofv3 (1 first visit + 20
    timed-shape updates per kernel), or a note why not."""
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return {"note": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="scene_tracks_prof_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "st", "--", sys.executable,
                            os.path.abspath(__file__), "--kernels-only", "--workload", str(k)], capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"note": "rocprofv3 run failed (rc %d): %s" % (r.returncode, (r.stderr or "")[-300:])}
        res = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "")
            m = re.search(r"(tracks_\w+_kernel|assign_max_kernel)(<[^>]*>)?", name)
            if m:
                key = m.group(1) + (m.group(2) or "")
                res[key] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                            "max_us": float(row["MaxNs"]) / 1e3}
        return res or {"note": "no tracker kernel in the profiler's table"}
    except (OSError, subprocess.SubprocessError) as e:
        return {"note": "rocprofv3 run failed: %r" % (e,)}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def kernel_resources(path):
    """Register / LDS / scratch figures of every kernel of csrc/tracks.hip from hipcc's resource remarks; {kernel: {...}} or None."""
    src = os.path.join(ROOT, "parq_amd", "csrc", "tracks.hip")
    hipcc = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc")
    try:
        err = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", "-o", os.devnull,
                              "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True, timeout=600, check=True).stderr
    except (OSError, subprocess.SubprocessError):
        return None
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() if shutil.which("c++filt") else m.group(2)
            cur = re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "")).replace("parq::", "").replace("void ", "")
            res[cur] = {}
        elif cur is not None:
            res[cur][m.group(1)] = int(m.group(2))
    if path:
        with open(path, "w") as f:
            f.write("hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage parq_amd/csrc/tracks.hip\n")
            for name, d in res.items():
                f.write("%s\n" % name)
                for k, v in d.items():
                    f.write("    %-28s %d\n" % (k, v))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--workload", type=int, default=0)
    ap.add_argument("--no-profiler", action="store_true")
    a = ap.parse_args()
    if a.kernels_only:
        return kernels_only(a.workload)
    # child processes of their own, one per workload, before this process opens the GPU
    prof = [{"note": "skipped"} if a.no_profiler else profiler_kernels(k) for k in range(len(WORKLOADS))]
    import torch
    from parq_amd import SceneTracks
    from parq_amd.f1_eval import F1Calculator
    rec = {"box": {"gpu": None}, "workloads": [], "kernel_resources": kernel_resources(a.resources)}
    rec["box"] = {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName}
    for k, w in enumerate(WORKLOADS):
        first, second = inputs(w)
        none = [{"labels": torch.zeros(0, dtype=torch.int64), "gt_corners_world": torch.zeros(0, 8, 3)} for _ in range(w["scenes"])]
        calc = F1Calculator(0.1, iou_device="cuda")
        calc.step(first, none)
        saved_host = copy.deepcopy(calc.preds)
        tracks = SceneTracks(max_tracks=512)
        feed(tracks, first)
        saved_dev = tracks._store.clone()
        wall = {"host_tracker": [], "device_tracker": []}
        dev_ms = []
        for rep in range(a.repeats + 1):                                  # the first repeat warms up and is dropped
            calc.preds = copy.deepcopy(saved_host)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calc.step(second, none)
            torch.cuda.synchronize()
            wall["host_tracker"].append((time.perf_counter() - t0) * 1e3)
            tracks._store.copy_(saved_dev)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            feed(tracks, second)
            e1.record()
            torch.cuda.synchronize()
            wall["device_tracker"].append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(e0.elapsed_time(e1))
        got = tracks.to_host()
        for n, trks in calc.preds.items():
            assert sorted_tracks(got[n]) == sorted_tracks(trks), "the two trackers left different tracks in %s" % n
        assert not any(tracks.dropped().values())
        wall = {k: v[1:] for k, v in wall.items()}
        dev_ms = dev_ms[1:]
        med = {k: statistics.median(v) for k, v in wall.items()}
        spread = max(max(v) - min(v) for v in wall.values())
        gain = med["host_tracker"] - med["device_tracker"]
        row = {"workload": "%d scenes x %d detections x %d tracks, seed %d, prediction side of one step" % (w["scenes"], w["dets"], w["tracks"], w["seed"]),
               "tracks_after": {n: len(t) for n, t in got.items()},
               "wall_ms": {"what": "host wall time of one step ending in torch.cuda.synchronize(), paths alternating, %d repeats" % a.repeats,
                           "host_tracker": wall["host_tracker"], "device_tracker": wall["device_tracker"], "median": med,
                           "repeat_spread_ms": spread, "host_minus_device_ms": gain, "gain_exceeds_spread": bool(gain > spread)},
               "device_ms": {"what": "device time of one SceneTracks.update between two stream events", "values": dev_ms,
                             "median": statistics.median(dev_ms)},
               "kernels_rocprofv3": {"what": "per-kernel times of a separate rocprofv3 --kernel-trace --stats run of this workload: 20 "
                                             "updates and the first visit that fills the store", "kernels": prof[k]}}
        rec["workloads"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({"kernel_resources": rec["kernel_resources"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
