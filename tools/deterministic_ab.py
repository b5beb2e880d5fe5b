"""Cost of deterministic mode: the `bench.py --train` step with and without torch.use_deterministic_algorithms(True), in alternating
fresh processes on one GPU (include/parq_hip.h parq_set_deterministic).

    python tools/deterministic_ab.py [--repeats 3] [--steps 10] [--warmup 3] [--token-grad] [--out profiles/deterministic_ab.json]

Each repeat runs the default step, then the deterministic one, each in a child process of its own (bench.py unchanged, switched on
by the child before bench.py's main runs); the JSON record lists every ms/step and the ratio of the medians.  Deterministic mode
also makes torch fill every torch.empty with NaN (torch.utils.deterministic.fill_uninitialized_memory): that is part of what a
user who switches it on pays, and part of the number."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CHILD = """
import runpy, sys, torch
torch.use_deterministic_algorithms(%s)
sys.argv = ["bench.py", "--gpus", "1", "--train", "--steps", "%d", "--warmup", "%d"] + %r
runpy.run_path("bench.py", run_name="__main__")
"""


def one(det, steps, warmup, extra):
    r = subprocess.run([sys.executable, "-c", CHILD % (det, steps, warmup, extra)], cwd=ROOT, capture_output=True, text=True, timeout=1200)
    if r.returncode != 0:
        raise RuntimeError("bench child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    d = json.loads(line)
    return d["ms_per_step"], d["final_loss"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--token-grad", action="store_true", help="also d loss / d tokens (runs the token-gradient gather)")
    a = ap.parse_args()
    rows = {"default": [], "deterministic": []}
    for _ in range(a.repeats):
        for name, det in (("default", False), ("deterministic", True)):
            ms, loss = one(det, a.steps, a.warmup, ["--token-grad"] if a.token_grad else [])
            rows[name].append(ms)
            print("%-13s %.3f ms/step  loss %.6f" % (name, ms, loss), flush=True)
    med = {k: statistics.median(v) for k, v in rows.items()}
    rec = {"workload": "bench.py --train%s (BASELINE cfg4 per-GPU shard), alternating fresh processes" % (" --token-grad" if a.token_grad else ""),
           "steps": a.steps,
           "warmup": a.warmup, "ms_per_step": rows, "median_ms": med, "ratio_deterministic_over_default": med["deterministic"] / med["default"]}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
