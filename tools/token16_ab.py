"""A/B of 16-bit memory tokens in the inference forward (include/parq_hip.h parq_set_token_type) at BASELINE cfg 2, 3 and 5.

Three variants of one forward, alternated within each round (3 rounds), timed with device events around the whole call:
  fp32      fp32 tokens;
  bf16-up   bf16 tokens upcast with .to(torch.float32) in front of the fp32-token forward — what PARQDecoder did with 16-bit tokens
            before they were taken natively (the copy is made inside the timed call, as it was);
  bf16      bf16 tokens passed through as they are.
Per variant: median forward time and the rise of torch.cuda.max_memory_allocated() over the pre-call memory_allocated().
Prints one JSON line per configuration (and with --ray-pe one per configuration for AddRayPE.tokens).  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/token16_ab.py
--configs cfg3 --rounds 1` (a run of its own)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {      # BASELINE.json: views, feature map, queries, iterations, cross-attention mode of the benchmark line
    "cfg2": dict(views=5, hw=(120, 160), queries=128, iters=4, mode="bf16"),
    "cfg3": dict(views=10, hw=(120, 160), queries=256, iters=8, mode=None),
    "cfg5": dict(views=20, hw=(240, 320), queries=512, iters=12, mode="fp16"),
}


def build(name, device):
    from parq_amd import synth
    from parq_amd.decoder import PARQDecoder
    c = CONFIGS[name]
    cfg = synth.decoder_cfg(dim=256, queries=c["queries"], heads=4, ffn=768, layers=c["iters"])
    W = synth.make_decoder_weights(cfg, seed=2024)
    dec = PARQDecoder(cfg).eval()
    sd = dec.state_dict()
    for k in sd:
        sd[k] = torch.from_numpy(W[k.replace("parq_module.decoder.mlp_heads.", "mlp_heads.")]).reshape(sd[k].shape)
    dec.load_state_dict(sd, strict=True)
    dec = dec.to(device)
    if c["mode"]:
        dec.attention_mode = c["mode"]
    h, w = c["hw"]
    cam, T_cp, T_wp, T_wl = synth.make_geometry(11, 1, c["views"], h, w)
    g = torch.Generator(device=device).manual_seed(11)
    tokens = torch.randn(1, c["views"] * h * w, 256, device=device, generator=g)
    geo = tuple(torch.from_numpy(a).to(device) for a in (cam, T_cp, T_wp, T_wl))
    return dec, tokens, geo, (h, w)


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    del out
    return a.elapsed_time(b), rise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg3,cfg5")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per variant and round")
    ap.add_argument("--ray-pe", action="store_true", help="also AddRayPE.tokens: fp32, fp32 then .to(bf16), bf16 from the kernel")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in args.configs.split(","):
        dec, t32, geo, hw = build(name, dev)
        t16 = t32.to(torch.bfloat16)
        variants = {"fp32": lambda: dec(t32, *geo, feat_hw=hw),
                    "bf16-up": lambda: dec(t16.to(torch.float32), *geo, feat_hw=hw),
                    "bf16": lambda: dec(t16, *geo, feat_hw=hw)}
        ms = {k: [] for k in variants}
        mem = {k: 0 for k in variants}
        with torch.no_grad():
            for fn in variants.values():          # warm-up: workspaces, graphs captured per key
                for _ in range(3):
                    fn()
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    for _ in range(args.calls):
                        t, r = timed(fn)
                        ms[k].append(t)
                        mem[k] = max(mem[k], r)
        line = {"config": name, "mode": dec.attention_mode, "tokens": list(t32.shape), "rounds": args.rounds, "calls": args.calls}
        for k in variants:
            line[k] = {"median_ms": round(statistics.median(ms[k]), 4), "min_ms": round(min(ms[k]), 4),
                       "peak_rise_mb": round(mem[k] / 1e6, 1)}
        print(json.dumps(line), flush=True)
        del dec, t32, t16
        torch.cuda.empty_cache()
    if args.ray_pe:
        for name in args.configs.split(","):
            ray_pe_ab(name, dev, args.rounds, args.calls)


def ray_pe_ab(name, device, rounds, calls):
    """AddRayPE.tokens at a configuration's geometry: fp32 tokens, fp32 tokens converted with .to(bf16), bf16 tokens from the kernel."""
    from parq_amd import AddRayPE, synth
    c = CONFIGS[name]
    h, w = c["hw"]
    pe = AddRayPE(256, synth.DEFAULT_SCALE, 64, 0.25, 5.25)
    pe.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_ray_pe_weights(256, 5).items()}, strict=True)
    pe = pe.to(device).eval()
    geo = tuple(torch.from_numpy(a).to(device) for a in synth.make_geometry(12, 1, c["views"], h, w))
    feat = torch.randn(1, c["views"], 256, h, w, device=device)
    variants = {"fp32": lambda: pe.tokens(feat, *geo),
                "fp32-to-bf16": lambda: pe.tokens(feat, *geo).to(torch.bfloat16),
                "bf16": lambda: pe.tokens(feat, *geo, dtype=torch.bfloat16)}
    ms = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():
            for _ in range(3):
                fn()
        for _ in range(rounds):
            for k, fn in variants.items():
                for _ in range(calls):
                    ms[k].append(timed(fn)[0])
    line = {"ray_pe": name, "tokens": [1, c["views"] * h * w, 256]}
    for k in variants:
        line[k] = {"median_ms": round(statistics.median(ms[k]), 4), "min_ms": round(min(ms[k]), 4)}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
