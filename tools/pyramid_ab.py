"""A/B of the FPN neck: AddRayPE.tokens_from_pyramid (resize gathered inside the ray-PE kernels, gather-form adjoint) against the
torch composition the reference runs (F.interpolate to level `layer` + torch.cat + AddRayPE.tokens), on the device.

Two geometries: the shipped one (3 views, 60x80 target, 4 x 256 channels) and a cfg-3-sized pyramid (10 views, 120x160 target,
4 x 64 channels).  Per geometry and path: an inference call (no_grad, eval mode) and a training step of the tokenisation node
(forward + backward into the encoder and the four levels), each timed with device events over `--iters` calls after `--warmup`
calls; the median of `--reps` such means is reported.  Writes one JSON document (default profiles/pyramid_ab.json).

    python tools/pyramid_ab.py [--out profiles/pyramid_ab.json] [--iters 20] [--warmup 5] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parq_amd import AddRayPE, Camera, Pose, synth  # noqa: E402

GEOMETRIES = {
    "shipped": dict(B=1, V=3, C=1024, layer=0, sizes=[(60, 80), (30, 40), (15, 20), (8, 10)]),
    "cfg3": dict(B=1, V=10, C=256, layer=0, sizes=[(120, 160), (60, 80), (30, 40), (15, 20)]),
}


def compose(levels, layer):
    B, V = levels[0].shape[:2]
    size = tuple(levels[layer].shape[-2:])
    return torch.cat([F.interpolate(lv.flatten(0, 1), size, mode="bilinear").unflatten(0, (B, V)) for lv in levels], 2)


def timed(fn, iters, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    means = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        means.append(a.elapsed_time(b) / iters)
    return statistics.median(means), min(means)


def run(name, g, args):
    B, V, C, layer = g["B"], g["V"], g["C"], g["layer"]
    h, w = g["sizes"][layer]
    torch.manual_seed(1)
    mod = AddRayPE(C).cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    cam, T_cp, T_wp, T_wl = synth.make_geometry(2, B, V, h, w)
    geo = (Camera(dev(cam)), Pose(dev(T_cp)), Pose(dev(T_wp)), Pose(dev(T_wl)))
    levels = [torch.randn(B, V, C // 4, hl, wl, device="cuda") * 0.5 for hl, wl in g["sizes"]]
    cot = torch.randn(B, V * h * w, C, device="cuda")
    out = {"geometry": dict(g, target=[h, w]), "tokens_MB": B * V * h * w * C * 4 / 1e6,
           "stack_MB": B * V * h * w * C * 4 / 1e6, "levels_MB": sum(lv.numel() for lv in levels) * 4 / 1e6}

    mod.eval()
    with torch.no_grad():
        fused = lambda: mod.tokens_from_pyramid(levels, layer, *geo)
        torchc = lambda: mod.tokens(compose(levels, layer), *geo)
        out["inference_ms"] = {"fused": timed(fused, args.iters, args.warmup, args.reps)[0],
                               "composition": timed(torchc, args.iters, args.warmup, args.reps)[0]}
    mod.train()
    leaves = [lv.clone().requires_grad_(True) for lv in levels]

    def train(fused_path):
        def step():
            mod.zero_grad(set_to_none=True)
            for lv in leaves:
                lv.grad = None
            tok = mod.tokens_from_pyramid(leaves, layer, *geo) if fused_path else mod.tokens(compose(leaves, layer), *geo)
            tok.backward(cot)
        return step
    out["train_fwd_bwd_ms"] = {"fused": timed(train(True), args.iters, args.warmup, args.reps)[0],
                               "composition": timed(train(False), args.iters, args.warmup, args.reps)[0]}
    # torch.use_deterministic_algorithms(True): the fused node's backward is the same; the composition raises, or takes torch's
    # deterministic fallback for the bilinear-interpolate backward
    torch.use_deterministic_algorithms(True)
    try:
        det = {"fused": timed(train(True), args.iters, args.warmup, args.reps)[0]}
        try:
            det["composition"] = timed(train(False), args.iters, args.warmup, args.reps)[0]
            det["speedup"] = det["composition"] / det["fused"]
        except RuntimeError as e:
            det["composition"] = "raises: %s" % str(e).splitlines()[0][:160]
    finally:
        torch.use_deterministic_algorithms(False)
    out["train_fwd_bwd_deterministic_ms"] = det
    for k in ("inference_ms", "train_fwd_bwd_ms"):
        out[k]["speedup"] = out[k]["composition"] / out[k]["fused"]
    print("%-8s inference fused %.3f ms  composition %.3f ms | train fwd+bwd fused %.3f ms  composition %.3f ms" % (
        name, out["inference_ms"]["fused"], out["inference_ms"]["composition"], out["train_fwd_bwd_ms"]["fused"],
        out["train_fwd_bwd_ms"]["composition"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_ab.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "warmup": args.warmup,
           "reps": args.reps, "timing": "device events around `iters` back-to-back calls, median of `reps` means",
           "results": {name: run(name, g, args) for name, g in GEOMETRIES.items()}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
