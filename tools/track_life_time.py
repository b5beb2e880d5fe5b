"""What the tracks' life costs per step: SceneTracks.update alone (lifecycle off: what the store did before it had a life), update +
note (lifecycle on), and update + note + retire (parq_amd/scene_tracks.py, include/parq_hip.h parq_tracks_note / parq_tracks_retire).

    python tools/track_life_time.py [--repeats 5] [--out profiles/track_life.json] [--resources profiles/track_life_kernel_resources.txt]
    python tools/track_life_time.py --resources-only --resources profiles/track_life_kernel_resources.txt       (needs no GPU)

The two workloads of tools/scene_tracks_time.py (4 scenes x 30 detections x 80 tracks and 8 x 64 x 400, seed 12).  Every scene holds
its tracks when the timed step arrives and every repeat starts from that state.  The three settings alternate in one process, five
repeats after a warm-up; the number is the host wall time of one step ending in a synchronise, and beside it the device time between
two stream events.  The retire of the timed step is one that has work to do: min_hits = 2, tentative_age = 0, so every track the step
did not match (about two in three) is removed and the matched ones move up.  An added time is called a cost only where it exceeds
the repeat spread.  The kernels' register / LDS / scratch figures, from the compiler's remarks for csrc/track_life.hip, go to
--resources."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from scene_tracks_time import WORKLOADS, feed, inputs  # noqa: E402

RETIRE = dict(min_hits=2, max_age=30, tentative_age=0)
SETTINGS = ("update", "update_note", "update_note_retire")


def kernel_resources(path):
    """Register / LDS / scratch figures of every kernel of csrc/track_life.hip from hipcc's resource remarks; {kernel: {...}} or None."""
    src = os.path.join(ROOT, "parq_amd", "csrc", "track_life.hip")
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
    assert all(d["ScratchSize [bytes/lane]"] == 0 for d in res.values()), res
    if path:
        with open(path, "w") as f:
            f.write("hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage parq_amd/csrc/track_life.hip\n")
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
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        print(json.dumps({"kernel_resources": kernel_resources(a.resources)}))
        return
    import torch
    from parq_amd import SceneTracks
    rec = {"box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName}, "retire": RETIRE,
           "workloads": [], "kernel_resources": kernel_resources(a.resources)}
    for w in WORKLOADS:
        first, second = inputs(w)
        plain, alive = SceneTracks(max_tracks=512), SceneTracks(max_tracks=512, lifecycle=True)
        feed(plain, first)
        feed(alive, first)
        saved = plain._store.clone(), alive._store.clone(), alive._life.clone()
        assert torch.equal(saved[0], saved[1])

        def step(setting):
            if setting == "update":
                plain._store.copy_(saved[0])
            else:
                alive._store.copy_(saved[1])
                alive._life.copy_(saved[2])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            feed(plain if setting == "update" else alive, second)
            if setting == "update_note_retire":
                alive.retire(**RETIRE)
            e1.record()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
        wall, dev_ms = {s: [] for s in SETTINGS}, {s: [] for s in SETTINGS}
        counts = {}
        for rep in range(a.repeats + 1):                                  # the first repeat warms up and is dropped
            for s in SETTINGS:
                ms, dms = step(s)
                wall[s].append(ms)
                dev_ms[s].append(dms)
                counts[s] = {n: len(t) for n, t in (plain if s == "update" else alive).to_host().items()}
        assert counts["update"] == counts["update_note"] and not any(plain.dropped().values())
        retired = {n: counts["update_note"][n] - counts["update_note_retire"][n] for n in counts["update"]}
        assert min(retired.values()) > 0
        wall = {s: v[1:] for s, v in wall.items()}
        dev_ms = {s: v[1:] for s, v in dev_ms.items()}
        med = {s: statistics.median(v) for s, v in wall.items()}
        spread = max(max(v) - min(v) for v in wall.values())
        added = {s: med[s] - med["update"] for s in SETTINGS[1:]}
        row = {"workload": "%d scenes x %d detections x %d tracks, seed %d, one step" % (w["scenes"], w["dets"], w["tracks"], w["seed"]),
               "tracks_after_update": counts["update"], "tracks_retired_by_the_timed_retire": retired,
               "wall_ms": {"what": "host wall time of one step ending in torch.cuda.synchronize(), the three settings alternating, %d repeats"
                                   % a.repeats, "values": wall, "median": med, "repeat_spread_ms": spread, "added_ms_over_update": added,
                           "added_exceeds_spread": {s: bool(v > spread) for s, v in added.items()}},
               "device_ms": {"what": "device time of the same step between two stream events", "values": dev_ms,
                             "median": {s: statistics.median(v) for s, v in dev_ms.items()}}}
        rec["workloads"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({"kernel_resources": rec["kernel_resources"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
