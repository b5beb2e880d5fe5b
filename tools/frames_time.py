"""Cost of preparing one snippet's raw frames on the device (parq_amd.resize_frames / FramePrep; include/parq_hip.h
parq_frames_resize) at the workload's own shape: 1 scene, 9 frames of 1296 x 968 -> 320 x 240 float32 under pad="scannet".

    python tools/frames_time.py [--window-ms 400] [--out profiles/frames_prep.json] [--bench-line '<bench.py JSON line>']

Items, on the device (device events around windows of back-to-back calls, every item as many calls as fill --window-ms (at least
20), three rounds in which the items take turns; "host_enqueue_ms" is what the host needs per call without waiting for the device):
  resize_frames   the one launch: reads 9 x 3.76 MB of bytes, writes 9 x 0.92 MB of float32;
  frame_prep      FramePrep as a whole: the launch plus the small tensor operations of intrinsics and poses;
  clone           a plain device copy (Tensor.clone) of the same input bytes: the stream rate the launch is to be judged against;
                  both get the bytes they have to move over their time;
  resize_uint8    the same launch writing bytes (output 4 times smaller);
  same_size       the launch on 9 frames of 320 x 240 -> 320 x 240 (identity plans, 3-word taps: the same grid, setup, staging
                  pattern and stores with next to no tap work): what of a call is not the two passes' arithmetic;
  upload_uint8    the raw frames from pinned host memory to the device (what the device path has to upload);
  upload_float    the float32 result from pinned host memory to the device (what the host path has to upload).
On the host, once per frame, if Pillow is installed: Image.resize + np.array(float32) + / 255 (the reference's ResizeImage +
Normalize), one core; otherwise the figure is reported as not measured here.  The outputs are checked against the NumPy statement of
the rule (tests/frames_cases.py) before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, T, W, H, w, h = 1, 9, 1296, 968, 320, 240


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


def host_path(frames, np):
    """Seconds per frame of the reference's host path, or None without Pillow: pad, Pillow resize, float32, / 255."""
    try:
        from PIL import Image, ImageOps
    except ImportError:
        return None, None
    outs, times = [], []
    for rep in range(2):                                   # the first round warms Pillow and the allocator
        for f in frames:
            t0 = time.perf_counter()
            im = ImageOps.expand(Image.fromarray(f, "RGB"), border=(0, 2))
            a = np.array(im.resize((w, h), Image.BILINEAR), dtype=np.float32) / 255
            if rep:
                times.append(time.perf_counter() - t0)
                outs.append(a.transpose(2, 0, 1))
    return statistics.mean(times), np.stack(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-line", default=None, help="the box's bench.py JSON result line, recorded alongside")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("frames_time.py measures on the GPU; none is visible")
    import frames_cases as FC
    from parq_amd.frames import FramePrep, resize_frames
    frames = FC.make_frames(B * T, W, H, seed=24).reshape(B, T, H, W, 3)
    K = np.tile(np.array([[1170.0, 0, 647.75], [0, 1170.0, 483.75], [0, 0, 1]]), (B, T, 1, 1))
    _, M = FC.case_poses(dict(B=B, T=T, inp=(W, H)))
    pinned = torch.from_numpy(frames).pin_memory()
    d = pinned.cuda()
    Kd, Md = torch.from_numpy(K).cuda(), torch.from_numpy(M).cuda()
    out = torch.empty(B, T, 3, h, w, device="cuda")
    pinned_f = torch.empty(B, T, 3, h, w).pin_memory()
    up8, upf = torch.empty_like(d), torch.empty_like(out)
    prep = FramePrep()
    out8 = torch.empty(B, T, 3, h, w, device="cuda", dtype=torch.uint8)
    small = torch.from_numpy(FC.make_frames(B * T, w, h, seed=25).reshape(B, T, h, w, 3)).cuda()

    want = FC.resize_statement(frames[0, :2], (0, 2, 0, 2), (w, h))
    got = resize_frames(d, out=out).cpu().numpy()
    if not np.array_equal(got[0, :2].view(np.uint32), FC.as_float(want).view(np.uint32)):
        raise SystemExit("resize_frames differs from the NumPy statement of the rule: nothing timed")
    host_s, host_out = host_path(frames[0], np)
    if host_out is not None and not np.array_equal(host_out.view(np.uint32), got[0].view(np.uint32)):
        raise SystemExit("resize_frames differs from Pillow's resize / 255: nothing timed")

    res = timed({"resize_frames": lambda: resize_frames(d, out=out),
                 "frame_prep": lambda: prep(d, Kd, Md),
                 "clone": lambda: d.clone(),
                 "resize_uint8": lambda: resize_frames(d, dtype=torch.uint8, out=out8),
                 "same_size": lambda: resize_frames(small, out=out),
                 "upload_uint8": lambda: up8.copy_(pinned, non_blocking=True),
                 "upload_float": lambda: upf.copy_(pinned_f, non_blocking=True)}, a.window_ms, torch)
    med = lambda k: statistics.median(res[k]["ms"])
    in_bytes, out_bytes = frames.size, 4 * B * T * 3 * h * w
    rec = {"what": "device-event time per CALL (host work of the call included), three windows of --window-ms of back-to-back calls each, "
                   "the items taking turns (ms)",
           "box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName},
           "shape": "%d scene, %d frames of %d x %d uint8 -> %d x %d float32, pad (0, 2, 0, 2)" % (B, T, W, H, w, h),
           "bit_equal_to_numpy_rule": True, "bit_equal_to_pillow": None if host_out is None else True}
    for k, v in res.items():
        rec[k + "_ms"] = v["ms"]
    rec["host_enqueue_ms"] = {k: v["host_enqueue_ms"] for k, v in res.items()}
    rec["calls_per_window"] = {k: v["calls_per_window"] for k, v in res.items()}
    rec["bytes"] = {"resize_frames": in_bytes + out_bytes, "clone": 2 * in_bytes, "upload_uint8": in_bytes, "upload_float": out_bytes}
    rec["GBps_of_needed_bytes"] = {k: rec["bytes"][k] / med(k) / 1e6 for k in rec["bytes"]}
    rec["resize_frames_over_clone"] = med("resize_frames") / med("clone")
    rec["tap_work_share_of_call"] = 1.0 - med("same_size") / med("resize_frames")
    if host_s is None:
        rec["host_pillow_ms_per_frame"] = None
        rec["host_pillow_note"] = ("Pillow is not installed on this box: not measured here (development machine, one core, warmed, mean "
                                   "of 10 calls: 12-14 ms per frame for the resize alone)")
    else:
        rec["host_pillow_ms_per_frame"] = host_s * 1e3
        rec["host_path_ms"] = {"pillow_resize_float_div": host_s * 1e3 * T, "upload_float": med("upload_float"),
                               "total": host_s * 1e3 * T + med("upload_float")}
        rec["host_path_over_device_path"] = rec["host_path_ms"]["total"] / (med("upload_uint8") + med("frame_prep"))
    rec["device_path_ms"] = {"upload_uint8": med("upload_uint8"), "frame_prep": med("frame_prep"),
                             "total": med("upload_uint8") + med("frame_prep")}
    if a.bench_line:
        rec["bench_py_headline"] = json.loads(a.bench_line)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
