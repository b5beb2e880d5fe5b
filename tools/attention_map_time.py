"""Cost of the cross-attention maps (PARQDecoder.cross_attention_map / cross_attention_view_mass; include/parq_hip.h
parq_attention_map) beside the reference's way to the same tensor, torch's multi_head_attention_forward(need_weights=True) on the
device from the same tokens (model/transformer_parq.py:377-380).

    python tools/attention_map_time.py [--window-ms 400] [--out profiles/attention_map.json]

Two geometries, one scene each: BASELINE cfg 3 (10 views of 120x160 features, 256 queries, d = 256, 4 heads: N = 192 000) and the
reference's shipped one (3 views of 60x80, 256 queries, d = 1024, 4 heads of 256: N = 14 400).  After one inference forward (seeded
synthetic weights and features) it times the full head-mean map, a 16-query map (its index tensor staged on the device once), the
view mass, the per-head map in fp16 — and torch's op.  The op gets the workspace's projected queries ("cross_q") through an identity
query in-projection and projects K and V from the tokens itself, as the reference's call does: the same Q K^T, softmax and head
mean (the record states how far the two maps are apart).

How: device events around a window of back-to-back calls; every item gets as many calls as fill --window-ms (at least 20), the
same rule for torch's op, and the items take turns — three rounds, each one window of every item — so that a drift of the clock
meets all of them alike.  The figures are CALL times: a call is five or six small launches behind a scratch allocation and the
Python of the method.  "host_enqueue_ms" is what the host needs per call without waiting for the device: where it is not well below
the call time, the call time is the host's and not the kernels'.
The record also states the bytes a full map has to move (the output once, K twice) and the rate that is of the measured time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

GEOMETRIES = {
    "cfg3": dict(views=10, feat_hw=(120, 160), queries=256, dim=256, heads=4, ffn=768),
    "shipped": dict(views=3, feat_hw=(60, 80), queries=256, dim=1024, heads=4, ffn=768),
}


def window(fn, n, torch):
    """(device ms per call, host ms per call to enqueue) of n back-to-back calls."""
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
    """fns: name -> callable.  name -> {"ms": [three windows], "host_enqueue_ms": .., "calls_per_window": ..}; the items alternate."""
    calls = {}
    for k, fn in fns.items():
        fn()
        fn()
        per, _ = window(fn, 5, torch)
        calls[k] = max(20, int(window_ms / per) + 1)
    res = {k: {"ms": [], "host_enqueue_ms": [], "calls_per_window": calls[k]} for k in fns}
    for _ in range(3):                                   # three rounds: the spread is part of the record
        for k, fn in fns.items():
            ms, host = window(fn, calls[k], torch)
            res[k]["ms"].append(ms)
            res[k]["host_enqueue_ms"].append(host)
    for k in res:
        res[k]["host_enqueue_ms"] = statistics.median(res[k]["host_enqueue_ms"])
    return res


def run(name, g, window_ms, torch):
    import torch.nn.functional as F
    from parq_amd import synth
    from parq_amd.decoder import PARQDecoder
    cfg = synth.decoder_cfg(dim=g["dim"], queries=g["queries"], heads=g["heads"], ffn=g["ffn"], layers=2)
    W = synth.make_decoder_weights(cfg, seed=2024)
    h, w = g["feat_hw"]
    sc = synth.make_scene(7, 1, g["views"], h, w, g["dim"], smooth=True)
    dec = PARQDecoder(cfg).eval()
    sd = dec.state_dict()
    for k in sd:
        sd[k] = torch.from_numpy(W[k.replace("parq_module.decoder.mlp_heads.", "mlp_heads.")]).reshape(sd[k].shape)
    dec.load_state_dict(sd, strict=True)
    dec = dec.cuda()
    dev = lambda a: torch.from_numpy(a).float().cuda()
    args = [dev(sc[k]) for k in ("tokens", "camera", "T_camera_pseudoCam", "T_world_pseudoCam", "T_world_local")]
    import warnings
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dec(*args, feat_hw=(h, w))
        dec.prepare(*args, feat_hw=(h, w))
        dec.iterate(0)
        torch.cuda.synchronize()
        C, H, Q, N = g["dim"], g["heads"], g["queries"], g["views"] * h * w
        out = torch.empty(1, Q, g["views"], h, w, device="cuda")
        out16 = torch.empty(1, H, Q, g["views"], h, w, device="cuda", dtype=torch.float16)
        sel = torch.tensor(list(range(0, Q, Q // 16))[:16], dtype=torch.int32, device="cuda")     # staged once: used as it is
        rec = {"geometry": "%d views %dx%d, Q = %d, d = %d, %d heads: N = %d" % (g["views"], h, w, Q, C, H, N),
               "attention_mode": dec.attention_mode, "safe_heads": dec.safe_heads}
        # torch's op from the same tokens: q = cross_q (identity rows for the query part of the in-projection), k, v projected by the op
        q = dec.intermediate("cross_q").view(1, Q, C).transpose(0, 1).contiguous()
        mem = args[0].transpose(0, 1).contiguous()
        p = "parq_module.decoder.layers.0.multihead_attn."
        in_w = dev(W[p + "in_proj_weight"]).clone()
        in_b = dev(W[p + "in_proj_bias"]).clone()
        in_w[:C] = torch.eye(C, device="cuda")
        in_b[:C] = 0
        ow, ob = dev(W[p + "out_proj.weight"]), dev(W[p + "out_proj.bias"])

        def torch_op():
            return F.multi_head_attention_forward(q, mem, mem, C, H, in_w, in_b, None, None, False, 0.0, ow, ob, training=False,
                                                  need_weights=True)[1]
        want = torch_op()
        got = dec.cross_attention_map().view(1, Q, N)
        torch.cuda.synchronize()
        rec["max_row_relative_difference_to_torch_fp32"] = float(((got - want).abs().amax(-1) / want.amax(-1)).max())
        t = timed({"full_map": lambda: dec.cross_attention_map(out=out),
                   "torch_mha_need_weights": torch_op,
                   "map_16_queries": lambda: dec.cross_attention_map(queries=sel),
                   "view_mass": lambda: dec.cross_attention_view_mass(),
                   "per_head_fp16": lambda: dec.cross_attention_map(per_head=True, dtype=torch.float16, out=out16)}, window_ms, torch)
        for k, v in t.items():
            rec[k + "_ms"] = v["ms"]
        rec["host_enqueue_ms"] = {k: v["host_enqueue_ms"] for k, v in t.items()}
        rec["calls_per_window"] = {k: v["calls_per_window"] for k, v in t.items()}
    med = lambda k: statistics.median(rec[k])
    # bytes of K per element as the kernels read it: hi + lo fp16, hi16 + the e4m3 residual of a mode-4 stage, fp32, one 16-bit value
    stages = dec.attention_mode == "split8" and N % 64 == 0 and C == 256 and dec.safe_heads == 0
    k_bytes = (3 if stages else {"split": 4, "split8": 4, "fp32": 4, "fp16": 2, "bf16": 2}[dec.attention_mode]) * N * C
    moved = 4 * Q * N + 2 * k_bytes
    rec["full_map_bytes"] = {"output": 4 * Q * N, "k_read_twice": 2 * k_bytes}
    rec["full_map_GBps_of_needed_bytes"] = moved / med("full_map_ms") / 1e6
    rec["torch_over_full_map"] = med("torch_mha_need_weights_ms") / med("full_map_ms")
    print(name, json.dumps(rec), flush=True)
    dec._ws.clear()
    del dec
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--only", choices=sorted(GEOMETRIES), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("attention_map_time.py measures on the GPU; none is visible")
    rec = {"what": "device-event time per CALL (host work of the method included), three windows of --window-ms of back-to-back calls "
                   "each, the items taking turns (ms); one scene",
           "box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName}}
    for name, g in GEOMETRIES.items():
        if a.only in (None, name):
            rec[name] = run(name, g, a.window_ms, torch)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
