"""A/B of 16-bit memory tokens in the training step (include/parq_hip.h parq_set_train_token_type) at the BASELINE cfg-4 shard
(4 scenes, 10 views 120 x 160, d = 256, 8 iterations, dropout 0.1) and, with --configs cfg4,shipped, one line at the shipped width
(d = 1024, 4 heads of 256, one scene).

One step = decoder forward under autograd + the set loss + backward (parameters require grad; --token-grad: the tokens too).  Four
variants, alternated within each round (3 rounds), timed with device events around the whole step:
  fp32      fp32 tokens;
  bf16-up   bf16 tokens upcast with .to(torch.float32) inside the timed step — what PARQDecoder did with 16-bit tokens in training
            before they were taken natively (the copy lives until the backward has run, as it did);
  bf16      bf16 tokens passed through as they are;
  fp16      fp16 tokens passed through as they are (the split-precision K/V weight gradient runs two products instead of three).
Per variant: median and minimum ms per step and the rise of torch.cuda.max_memory_allocated() over the pre-step memory_allocated().
Prints one JSON line per configuration.  Run it once per tree to compare trees (on a tree whose decoder upcasts 16-bit tokens itself
"bf16" and "fp16" measure that upcast).  Kernel times: `rocprofv3 --kernel-trace --stats -- python tools/train_token16_ab.py
--rounds 1 --steps 2` (a run of its own); the template argument of kvproj_bwd_split_kernel is the token type (0 fp32, 1 fp16, 2 bf16)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {      # scenes, views, feature map, width, heads, ffn, queries, iterations
    "cfg4": dict(scenes=4, views=10, hw=(120, 160), dim=256, heads=4, ffn=768, queries=256, iters=8),
    "shipped": dict(scenes=1, views=10, hw=(120, 160), dim=1024, heads=4, ffn=1024, queries=256, iters=8),
}


def build(name, device):
    from parq_amd import Obb3D, PARQDecoder, Pose, synth
    c = CONFIGS[name]
    cfg = synth.decoder_cfg(dim=c["dim"], queries=c["queries"], heads=c["heads"], ffn=c["ffn"], layers=c["iters"], dropout=0.1)
    W = synth.make_decoder_weights(cfg, 41, damped=True)
    dec = PARQDecoder(cfg)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=False)
    dec = dec.to(device).train()
    h, w = c["hw"]
    B = c["scenes"]
    cam, T_cp, T_wp, T_wl = synth.make_geometry(11, B, c["views"], h, w)
    g = torch.Generator(device=device).manual_seed(11)
    tokens = torch.randn(B, c["views"] * h * w, c["dim"], device=device, generator=g)
    geo = tuple(torch.from_numpy(a).to(device) for a in (cam, T_cp, T_wp, T_wl))
    obbs, sym = synth.make_boxes(3000, B, 12)
    target = (Obb3D(torch.from_numpy(obbs).to(device)), Pose(geo[3]), torch.from_numpy(sym).to(device))
    return dec, tokens, geo, (h, w), target


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg4")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per variant and round")
    ap.add_argument("--token-grad", action="store_true", help="the tokens require grad too (a trained backbone in front of the decoder)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    np.random.seed(1)
    for name in args.configs.split(","):
        dec, t32, geo, hw, (obbs, T_wl, sym) = build(name, dev)
        tb, th = t32.to(torch.bfloat16), t32.to(torch.float16)

        def step(make_tokens):
            dec.zero_grad(set_to_none=True)
            t = make_tokens()
            if args.token_grad:
                t = t.detach().requires_grad_(True)
            outs = dec(t, *geo, feat_hw=hw)
            dec.loss(outs, obbs, T_wl, sym)["total_loss"].backward()

        variants = {"fp32": lambda: step(lambda: t32),
                    "bf16-up": lambda: step(lambda: tb.to(torch.float32)),
                    "bf16": lambda: step(lambda: tb),
                    "fp16": lambda: step(lambda: th)}
        ms = {k: [] for k in variants}
        per_round = {k: [] for k in variants}
        mem = {k: 0 for k in variants}
        for fn in variants.values():              # warm-up: training workspaces, the allocator's steady state
            for _ in range(2):
                fn()
        for _ in range(args.rounds):
            for k, fn in variants.items():
                got = []
                for _ in range(args.steps):
                    t, r = timed(fn)
                    got.append(t)
                    mem[k] = max(mem[k], r)
                ms[k] += got
                per_round[k].append(statistics.median(got))
        dec.zero_grad(set_to_none=True)
        line = {"config": name, "train_mode": dec._train_mode(), "tokens": list(t32.shape), "rounds": args.rounds, "steps": args.steps,
                "token_grad": bool(args.token_grad)}
        for k in variants:
            line[k] = {"median_ms": round(statistics.median(ms[k]), 3), "min_ms": round(min(ms[k]), 3),
                       "round_medians_ms": [round(x, 3) for x in per_round[k]], "peak_rise_mb": round(mem[k] / 1e6, 1)}
        print(json.dumps(line), flush=True)
        del dec, t32, tb, th
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
