"""Cost of drawing the detections of one snippet on the device (parq_amd.draw_boxes; include/parq_hip.h parq_draw_boxes) at the
workload's own shape: 1 scene, 10 views of 480 x 640, 256 boxes of which about 30 are kept.

    python tools/draw_boxes_time.py [--window-ms 400] [--out profiles/draw_boxes.json]

Beside the call it times
  (a) a plain device copy of the same images (Tensor.clone) — the stream rate the image-sized raster launch is to be judged against;
      both get the bytes they have to move (draw: the images read twice, by the min / max launch and by the raster launch, and the
      output written once; clone: read once, written once) over their time;
  (b) the NumPy statement of the rule (tests/draw_cases.py) on the host for the same inputs, once;
and, to say where the time of a call goes, the same call with M = 0 boxes (min / max + raster with nothing to cull or scan) and with
uint8 output.  How: device events around windows of back-to-back calls, every item as many calls as fill --window-ms (at least 20),
three rounds in which the items take turns; "host_enqueue_ms" is what the host needs per call without waiting for the device.  The
outputs are checked against the NumPy statement before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, T, H, W, M, KEPT, NSEM = 1, 10, 480, 640, 256, 30, 9


def make_inputs(seed, np):
    """Views on a slow arc around a room of M boxes (ScanNet-like intrinsics); KEPT boxes pass the mask, the rest would not."""
    rng = np.random.default_rng(seed)
    cam = np.zeros((B, T, 6), np.float32)
    cam[..., :] = [W, H, 577.0, 577.0, (W - 1) / 2.0, (H - 1) / 2.0]
    T_wp, T_cp = np.zeros((B, T, 12), np.float32), np.zeros((B, T, 12), np.float32)
    for t in range(T):
        a = 0.06 * (t - T / 2)
        T_wp[0, t, :9] = [np.cos(a), 0, np.sin(a), 0, 1, 0, -np.sin(a), 0, np.cos(a)]
        T_wp[0, t, 9:] = [0.1 * t - 0.5, 0.02 * t, 0.0]
        T_cp[0, t, :9] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    sign = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.float64) - 0.5
    corners = np.zeros((B, M, 8, 3), np.float32)
    for m in range(M):
        depth = rng.uniform(1.5, 4.0)
        centre = np.array([rng.uniform(-0.45, 0.45) * depth, rng.uniform(-0.3, 0.3) * depth, depth])
        ang = rng.uniform(-np.pi, np.pi)
        Ry = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        corners[0, m] = ((sign * rng.uniform(0.2, 1.0, 3)) @ Ry.T + centre).astype(np.float32)
    labels = rng.integers(0, NSEM, (B, M)).astype(np.int32)
    keep = np.zeros((B, M), bool)
    keep[0, rng.choice(M, KEPT, replace=False)] = True
    images = rng.standard_normal((B, T, 3, H, W)).astype(np.float32)
    return dict(images=images, camera=cam, T_cp=T_cp, T_wp=T_wp, corners=corners, labels=labels, keep=keep)


def window(fn, n, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    host = time.perf_counter() - t0
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n, host * 1e3 / n


def timed(fns, window_ms, torch):
    calls = {}
    for k, fn in fns.items():
        fn()
        fn()
        per, _ = window(fn, 5, torch)
        calls[k] = max(20, int(window_ms / per) + 1)
    res = {k: {"ms": [], "host_enqueue_ms": [], "calls_per_window": calls[k]} for k in fns}
    for _ in range(3):
        for k, fn in fns.items():
            ms, host = window(fn, calls[k], torch)
            res[k]["ms"].append(ms)
            res[k]["host_enqueue_ms"].append(host)
    for k in res:
        res[k]["host_enqueue_ms"] = statistics.median(res[k]["host_enqueue_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("draw_boxes_time.py measures on the GPU; none is visible")
    import draw_cases as D
    from parq_amd.draw import box_colors, draw_boxes
    sc = make_inputs(2025, np)
    d = {k: torch.from_numpy(v).cuda() for k, v in sc.items()}
    none = (torch.zeros(B, 0, 8, 3, device="cuda"), torch.zeros(B, 0, dtype=torch.int32, device="cuda"))
    view = (d["images"], d["camera"], d["T_cp"], d["T_wp"])
    out = torch.empty(B, 3, T * H, W, device="cuda")
    out8 = torch.empty(B, 3, T * H, W, device="cuda", dtype=torch.uint8)

    t0 = time.perf_counter()
    want, covered = D.draw_oracle(sc["images"], sc["camera"], sc["T_cp"], sc["T_wp"], sc["corners"], sc["labels"], sc["keep"], None,
                                  box_colors(NSEM), NSEM + 1)
    numpy_s = time.perf_counter() - t0
    got = draw_boxes(*view, d["corners"], d["labels"], d["keep"], num_semcls=NSEM, out=out).cpu().numpy()
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        raise SystemExit("draw_boxes differs from the NumPy statement of the rule: nothing timed")
    segs = sum(len(D.view_segments(sc["camera"][0, t], sc["T_cp"][0, t], sc["T_wp"][0, t], sc["corners"][0], sc["labels"][0], sc["keep"][0], None,
                                   NSEM + 1)) for t in range(T))

    res = timed({"draw_boxes": lambda: draw_boxes(*view, d["corners"], d["labels"], d["keep"], num_semcls=NSEM, out=out),
                 "clone": lambda: d["images"].clone(),
                 "draw_boxes_no_boxes": lambda: draw_boxes(*view, *none, num_semcls=NSEM, out=out),
                 "draw_boxes_uint8": lambda: draw_boxes(*view, d["corners"], d["labels"], d["keep"], num_semcls=NSEM, dtype=torch.uint8, out=out8)},
                a.window_ms, torch)
    med = lambda k: statistics.median(res[k]["ms"])
    img_bytes = 4 * B * T * 3 * H * W
    rec = {"what": "device-event time per CALL (host work of draw_boxes included), three windows of --window-ms of back-to-back calls each, "
                   "the items taking turns (ms)",
           "box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName},
           "shape": "%d scene, %d views of %d x %d, %d boxes, %d kept; %d drawn segments, %d covered pixels"
                    % (B, T, H, W, M, KEPT, segs, int(covered.sum())),
           "bit_equal_to_numpy_rule": True}
    for k, v in res.items():
        rec[k + "_ms"] = v["ms"]
    rec["host_enqueue_ms"] = {k: v["host_enqueue_ms"] for k, v in res.items()}
    rec["calls_per_window"] = {k: v["calls_per_window"] for k, v in res.items()}
    rec["bytes"] = {"draw_boxes": 3 * img_bytes, "clone": 2 * img_bytes}
    rec["GBps_of_needed_bytes"] = {"draw_boxes": 3 * img_bytes / med("draw_boxes") / 1e6, "clone": 2 * img_bytes / med("clone") / 1e6}
    rec["numpy_rule_on_host_s"] = numpy_s
    rec["draw_boxes_over_clone"] = med("draw_boxes") / med("clone")
    rec["numpy_over_draw_boxes"] = numpy_s * 1e3 / med("draw_boxes")
    rec["boxes_share_of_call"] = 1.0 - med("draw_boxes_no_boxes") / med("draw_boxes")
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
