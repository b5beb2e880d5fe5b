"""What a streaming view window (parq_amd.ViewWindow, include/parq_hip.h parq_forward_views) saves per forward, measured.

    python tools/view_window_ab.py [--forwards 200] [--repeats 3] [--only cfg3_b1] [--out profiles/view_window_ab.json]

One process; the variants of a shape take turns, --repeats rounds of --forwards forwards each after a warm-up of every variant; the
time is wall clock around a device synchronise, divided by the forwards.  Shapes: BASELINE cfg 3 (10 views of 120x160 features,
d = 256, 256 queries) and the reference's shipped geometry (3 views of 60x80, d = 1024), each with 1 and 4 scenes.  Variants:

  a  decoder.forward on the assembled tensors (every view projected)
  b  window.forward with all slots dirty (win.invalidate() in front of it: the same projection through the window, no copy)
  b_put   the same with a put of every view in front of it (the copy of all tokens into the window's buffer is inside the time)
  c  window.forward with ONE slot replaced per step (the slot rotates; the put's copy of that view's tokens is inside the time)
  put_one the put of c alone (one view's tokens, camera and poses copied into the slot)
  d_all   the module path without a window: AddRayPE.tokens over all views + a
  d_one   the module path with one: put_features of one view (its tokenisation only) + c's forward

Every repeat is recorded, with the spread (max - min) between the repeats of a variant and the token rows per scene each variant's
K/V projection covered.  Default policy of the decoder (range_check = "sync") unless --policy says otherwise."""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = {
    "cfg3_b1": dict(B=1, views=10, feat_hw=(120, 160), queries=256, dim=256, heads=4, ffn=768),
    "cfg3_b4": dict(B=4, views=10, feat_hw=(120, 160), queries=256, dim=256, heads=4, ffn=768),
    "shipped_b1": dict(B=1, views=3, feat_hw=(60, 80), queries=256, dim=1024, heads=4, ffn=768),
    "shipped_b4": dict(B=4, views=3, feat_hw=(60, 80), queries=256, dim=1024, heads=4, ffn=768),
}


def run(name, g, forwards, repeats, policy, torch):
    from types import SimpleNamespace as NS
    from parq_amd import PARQ, synth
    B, V, (h, w), Cd = g["B"], g["views"], g["feat_hw"], g["dim"]
    hw = h * w
    dcfg = synth.decoder_cfg(dim=Cd, queries=g["queries"], heads=g["heads"], ffn=g["ffn"], layers=8)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg))
    model = PARQ(cfg).eval()
    W, Wp = synth.make_decoder_weights(dcfg, 2024, damped=True), synth.make_ray_pe_weights(Cd, 2025)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("box3d_decoder."):
            sd[k] = torch.from_numpy(W[k[len("box3d_decoder."):].replace("parq_module.decoder.mlp_heads.", "mlp_heads.")]).reshape(sd[k].shape)
        else:
            sd[k] = torch.from_numpy(Wp[k[len("add_ray_pe."):]])
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    dec, pe = model.box3d_decoder, model.add_ray_pe
    dec.range_check = policy
    dev = lambda a: torch.from_numpy(a).float().cuda()
    cam, T_cp, T_wp, T_wl = (dev(a) for a in synth.make_geometry(7, B, V, h, w))
    # smooth feature maps of O(1), one view's worth, repeated over the views and scenes with a per-view scale (the values are irrelevant
    # to the time; they only have to stay inside every mode's range)
    one = dev(synth.make_tokens(8, 1, 1, h, w, Cd, smooth=True)).view(h, w, Cd).permute(2, 0, 1).contiguous()
    scale = torch.linspace(0.5, 1.0, B * V, device="cuda").view(B, V, 1, 1, 1)
    feats = (one.view(1, 1, Cd, h, w) * scale).contiguous()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tokens = pe.tokens(feats, cam, T_cp, T_wp, T_wl)
        win = dec.view_window(B, V, h, w, T_wl)
        mwin = model.view_window(B, V, h, w, T_wl)
        allv = list(range(V))
        state = {"slot": 0}
        rows = {}

        def a():
            dec(tokens, cam, T_cp, T_wp, T_wl, feat_hw=(h, w))

        def b():
            win.invalidate()
            win.forward()
            rows["b"] = win.last_projected_rows

        def b_put():
            win.put(allv, tokens, cam, T_cp, T_wp)
            win.forward()
            rows["b_put"] = win.last_projected_rows

        def put_one():
            s = state["slot"] = (state["slot"] + 1) % V
            win.put(s, tokens[:, s * hw:(s + 1) * hw], cam[:, s:s + 1], T_cp[:, s:s + 1], T_wp[:, s:s + 1])

        def c():
            s = state["slot"] = (state["slot"] + 1) % V
            win.put(s, tokens[:, s * hw:(s + 1) * hw], cam[:, s:s + 1], T_cp[:, s:s + 1], T_wp[:, s:s + 1])
            win.forward()
            rows["c"] = win.last_projected_rows

        def d_all():
            dec(pe.tokens(feats, cam, T_cp, T_wp, T_wl), cam, T_cp, T_wp, T_wl, feat_hw=(h, w))

        def d_one():
            s = state["slot"] = (state["slot"] + 1) % V
            mwin.put_features(s, feats[:, s:s + 1], cam[:, s:s + 1], T_cp[:, s:s + 1], T_wp[:, s:s + 1])
            mwin.forward()
            rows["d_one"] = mwin.last_projected_rows
        mwin.put_features(allv, feats, cam, T_cp, T_wp)
        win.put(allv, tokens, cam, T_cp, T_wp)
        variants = {"a": a, "b": b, "b_put": b_put, "c": c, "put_one": put_one, "d_all": d_all, "d_one": d_one}
        for fn in variants.values():                         # warm-up of every variant: packs, workspaces, graph captures, tier moves
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(repeats):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(forwards):
                    fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / forwards)
    N = V * hw
    rows.update({"a": N, "d_all": N, "put_one": 0})
    med = lambda k: sorted(ms[k])[len(ms[k]) // 2]
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    rec = {"geometry": "%d scene(s), %d views %dx%d, Q = %d, d = %d: N = %d" % (B, V, h, w, g["queries"], Cd, N),
           "attention_mode": dec.attention_mode, "safe_heads": dec.safe_heads, "range_check": policy, "iterations": 8,
           "forwards_per_repeat": forwards, "ms_per_forward": ms, "spread_ms": spread, "rows_projected_per_scene": rows,
           "replays": {"window": win._entry.replays, "module_window": mwin._entry.replays},
           "b_minus_a_us": (med("b") - med("a")) * 1e3, "a_minus_c_us": (med("a") - med("c")) * 1e3,
           "a_minus_c_percent": 100.0 * (med("a") - med("c")) / med("a"),
           "d_all_minus_d_one_us": (med("d_all") - med("d_one")) * 1e3,
           "d_all_minus_d_one_percent": 100.0 * (med("d_all") - med("d_one")) / med("d_all")}
    print(name, json.dumps(rec), flush=True)
    win.close()
    mwin.close()
    dec._ws.clear()
    del model, dec, win, mwin, tokens, feats
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forwards", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=sorted(SHAPES), action="append", default=None)
    ap.add_argument("--policy", choices=["sync", "lazy", "off"], default="sync")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.forwards < 200 or a.repeats < 3:
        print("note: fewer than 3 repeats of 200 forwards is a smoke run, not a record", file=sys.stderr)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("view_window_ab.py measures on the GPU; none is visible")
    rec = {"what": "wall-clock ms per forward around a device synchronise; variants a / b / b_put / c / put_one / d_all / d_one of tools/view_window_ab.py take "
                   "turns, every repeat listed",
           "box": {"gpu": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName}}
    for name, g in SHAPES.items():
        if a.only is None or name in a.only:
            rec[name] = run(name, g, a.forwards, a.repeats, a.policy, torch)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
