"""Cost of one snippet-targets call (parq_amd.SnippetTargets; include/parq_hip.h parq_snippet_targets) at the workload's own shape:
4 scenes, 3 frames of 480 x 640 uint16 depth, 40 boxes per scene, colour image 968 x 1296.

    python tools/snippet_targets_time.py [--repeats 5] [--calls 20] [--out profiles/snippet_targets.json] [--no-host]
    python tools/snippet_targets_time.py --trace-calls 50       # calls only, for a rocprofv3 --kernel-trace --stats run of its own

Wall time per call ENDING IN A SYNCHRONISE (host work of the call included), mean of --calls calls, for
  targets   SnippetTargets()(...): the two launches and the small uploads and allocations of the wrapper;
  c_abi     parq_snippet_targets alone on prepared device arguments: the two launches;
  clone     a device copy (Tensor.clone) of the same depth bytes: what a launch-bound call over these bytes costs at the least;
  host      the NumPy statement of the rule (tests/snippet_cases.py) on the host, one call per repeat.
The paths alternate, --repeats times.  By this project's rule a difference is a gain only if it exceeds the repeat spread: the record
carries every repeat, and ``separated`` says whether the slowest repeat of one path is below the fastest of the other.  The device
outputs are checked against the statement, bit for bit, before anything is timed."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASE = dict(name="workload", seed=31, B=4, T=3, depth=(480, 640), color=(968, 1296), n=(40, 40, 40, 40), S=50)


def per_call(fn, n, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy statement on the host (about 10 s per repeat)")
    ap.add_argument("--trace-calls", type=int, default=0, help="only make this many calls (for a kernel trace) and exit")
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("snippet_targets_time.py measures on the GPU; none is visible")
    import snippet_cases as SC
    from parq_amd import SnippetTargets, _lib
    d = SC.make_case(CASE)
    B, T, (Hd, Wd), N, S = CASE["B"], CASE["T"], CASE["depth"], 40, CASE["S"]
    depth = torch.from_numpy(d["depth"]).cuda()
    Kd, Kc = torch.from_numpy(d["depth_intrinsics"]), torch.from_numpy(d["color_intrinsics"])
    M, rows, sym = (torch.from_numpy(d[k]).cuda() for k in ("T_world_camera", "obbs", "sym"))
    tg = SnippetTargets()
    call = lambda: tg(depth, Kd, Kc, d["color_size"], M, rows, sym)
    if a.trace_calls:
        for _ in range(a.trace_calls):
            call()
        torch.cuda.synchronize()
        return

    # the bare entry point on prepared arguments
    lib = _lib.load()
    Ki = np.stack([np.linalg.inv(K) for K in d["depth_intrinsics"]])
    Ki_d, Kc_d = torch.from_numpy(Ki).cuda(), Kc.cuda()
    M12 = torch.cat([M[..., :3, :3].reshape(B, T, 9), M[..., :3, 3]], -1).contiguous()
    need = lib.parq_snippet_targets_workspace(B, T, Hd, Wd, N)
    mk = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")
    ws = mk((need,), torch.uint8)
    outs = [mk((B, 100, 19), torch.float32), mk((B, S), torch.float32), mk((B,), torch.int32), mk((B, T, N), torch.int32),
            mk((B, T, N), torch.float32), mk((B, N), torch.int32), mk((B, N), torch.float32), mk((B, N), torch.int32), mk((B, N), torch.int32)]
    p = lambda t: C.c_void_p(t.data_ptr())
    cnt, rat = (C.c_int32 * 3)(1000, 500, 100), (C.c_float * 3)(0.85, 0.70, 0.50)

    def abi():
        _lib.check(lib.parq_snippet_targets(p(depth), B, T, Hd, Wd, p(Ki_d), p(Kc_d), d["color_size"][0], d["color_size"][1], p(M12), p(rows),
                                            None, p(sym), 0, S, N, 100, cnt, rat, 3, 3, 1000.0, p(ws), need, *[p(o) for o in outs],
                                            _lib.stream_ptr()), "parq_snippet_targets")

    t0 = time.perf_counter()
    want = SC.statement(d["depth"], Ki, d["color_intrinsics"], d["color_size"], d["T_world_camera"], d["obbs"], d["sym"])
    first_host_s = time.perf_counter() - t0
    got = tg(depth, Kd, Kc, d["color_size"], M, rows, sym, details=True)
    abi()
    torch.cuda.synchronize()
    same = (np.array_equal(got["frame_points_inside"].cpu().numpy(), want["frame_points"])
            and np.array_equal(got["frame_truncation"].cpu().numpy().view(np.uint32), want["frame_truncation"].view(np.uint32))
            and np.array_equal(got["obbs_padded"]._data.cpu().numpy().view(np.uint32), want["obbs_padded"].view(np.uint32))
            and np.array_equal(outs[3].cpu().numpy(), want["frame_points"]) and np.array_equal(outs[2].cpu().numpy(), want["num_valid"]))
    if not same:
        raise SystemExit("the device outputs differ from the NumPy statement of the rule: nothing timed")

    paths = {"targets": call, "c_abi": abi, "clone": lambda: depth.clone()}
    for fn in paths.values():
        per_call(fn, 5, torch)
    ms = {k: [] for k in paths}
    host_ms = []
    for _ in range(a.repeats):
        for k, fn in paths.items():
            ms[k].append(per_call(fn, a.calls, torch))
        if not a.no_host:
            t0 = time.perf_counter()
            SC.statement(d["depth"], Ki, d["color_intrinsics"], d["color_size"], d["T_world_camera"], d["obbs"], d["sym"])
            host_ms.append((time.perf_counter() - t0) * 1e3)
    med = lambda v: statistics.median(v)
    sep = lambda lo, hi: max(lo) < min(hi)
    rec = {"what": "wall ms per call ending in a synchronise, mean of %d calls, %d repeats in which the paths alternate" % (a.calls, a.repeats),
           "box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName},
           "shape": "%d scenes, %d frames of %d x %d uint16, %d boxes per scene, colour %d x %d" % ((B, T, Wd, Hd, N) + d["color_size"][::-1]),
           "bit_equal_to_numpy_rule": True, "num_valid": want["num_valid"].tolist(), "depth_bytes": int(d["depth"].nbytes),
           "workspace_bytes": int(need),
           "targets_ms": ms["targets"], "c_abi_ms": ms["c_abi"], "clone_ms": ms["clone"],
           "host_statement_ms": host_ms if host_ms else None, "host_statement_first_call_ms": first_host_s * 1e3,
           "median_ms": {k: med(v) for k, v in ms.items()},
           "c_abi_over_clone": med(ms["c_abi"]) / med(ms["clone"]), "targets_over_clone": med(ms["targets"]) / med(ms["clone"]),
           "separated": {"clone_below_c_abi": sep(ms["clone"], ms["c_abi"]), "c_abi_below_targets": sep(ms["c_abi"], ms["targets"])}}
    if host_ms:
        rec["median_ms"]["host_statement"] = med(host_ms)
        rec["host_statement_over_targets"] = med(host_ms) / med(ms["targets"])
        rec["separated"]["targets_below_host_statement"] = sep(ms["targets"], host_ms)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
