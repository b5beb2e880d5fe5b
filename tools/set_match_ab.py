"""Cost or gain of matching on the device (PARQDecoder.match_on_device; include/parq_hip.h parq_set_match) in the training step of
`bench.py --train`: the BASELINE cfg-4 per-GPU shard (4 scenes, 10 views, 256 queries, 8 iterations, 12 boxes per scene).

    python tools/set_match_ab.py [--rounds 5] [--steps 20] [--warmup 3] [--out profiles/set_match_ab.json]
    python tools/set_match_ab.py --only on --rounds 1 --steps 6 --no-phases      # a short run with one setting, for a kernel trace

One process, one module, one optimizer.  The two settings ALTERNATE (off, on, off, on, ...): each round sets the flag, runs untimed
steps, synchronises, times `steps` steps with the host clock and synchronises before the clock is read; then five more steps with an
event between the phases give the device time of the `loss` phase (from the end of the forward's enqueue to the end of the loss's, host
stalls inside it included, as bench.py --phase-times measures it).  Medians over the rounds are reported with every round's value and
the spread (max - min) beside them; the project's rule: a difference smaller than the spread of either setting is "no gain"."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="both", choices=["both", "off", "on"])
    ap.add_argument("--no-phases", action="store_true", help="skip the event-delimited steps (a kernel trace then ends in plain steps)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from parq_amd import Obb3D, PARQDecoder, Pose, synth
    assert torch.cuda.is_available(), "tools/set_match_ab.py needs a GPU"
    device = torch.device("cuda", 0)
    Wl = bench.WORKLOAD
    B, V, (h, w), Q, C, I = 4, Wl["views"], Wl["feat_hw"], Wl["queries"], Wl["dim"], Wl["iters"]
    cfg = synth.decoder_cfg(dim=C, queries=Q, heads=Wl["heads"], ffn=Wl["ffn"], layers=I, dropout=0.1)
    dec = PARQDecoder(cfg)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_decoder_weights(cfg, 41, damped=True).items()}, strict=False)
    dec = dec.to(device).train()
    inputs = bench.build_inputs(B, device, seed=2000)
    obbs, sym = synth.make_boxes(3000, B, 12)
    obbs, sym = Obb3D(torch.from_numpy(obbs).to(device)), torch.from_numpy(sym).to(device)
    T_wl = Pose(inputs[4])
    opt = torch.optim.AdamW([p for p in dec.parameters() if p.requires_grad], lr=1e-4 * B / 256.0, foreach=True)
    np.random.seed(1)

    def step(ev=None):
        rec = (lambda i: ev[i].record()) if ev is not None else (lambda i: None)
        opt.zero_grad(set_to_none=True)
        rec(0); outs = dec(*inputs, feat_hw=(h, w))
        rec(1); loss = dec.loss(outs, obbs, T_wl, sym)["total_loss"]
        rec(2); loss.backward()
        torch.nn.utils.clip_grad_norm_(dec.parameters(), 1.0)
        opt.step()
        rec(3)
        return loss

    flags = {"both": (False, True), "off": (False,), "on": (True,)}[a.only]
    ms, loss_ms, steps_on = {f: [] for f in flags}, {f: [] for f in flags}, 0
    for flag in flags:                                   # spin-up under both settings, untimed
        dec.match_on_device = flag
        for _ in range(a.warmup):
            step()
    torch.cuda.synchronize()
    for rnd in range(a.rounds):
        for flag in flags:
            dec.match_on_device = flag
            before = dec._match_step
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step()
            torch.cuda.synchronize()
            ms[flag].append((time.perf_counter() - t0) / a.steps * 1e3)
            acc = []
            for _ in range(0 if a.no_phases else 5):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                step(ev)
                torch.cuda.synchronize()
                acc.append(ev[1].elapsed_time(ev[2]))
            loss_ms[flag].append(statistics.median(acc) if acc else float("nan"))
            assert (dec._match_step - before == a.steps + 2 + len(acc)) == flag, "the setting did not take the path it names"
            assert bool(torch.isfinite(loss))
    name = {False: "off", True: "on"}
    spread = lambda x: max(x) - min(x)
    rec = {"what": "training step of bench.py --train (cfg-4 shard: %d scenes, %d views, %d queries, %d iterations, 12 boxes per scene), "
                   "match_on_device off / on alternating in one process; ms per step = host clock around `steps` steps between two device "
                   "synchronisations; loss_phase_ms = device time between the events around PARQDecoder.loss; medians over `rounds`" % (B, V, Q, I),
           "rounds": a.rounds, "steps": a.steps, "gpu": torch.cuda.get_device_name(0), "train_attention_mode": dec._train_mode()}
    for f in flags:
        rec[name[f]] = {"ms_per_step": statistics.median(ms[f]), "ms_per_step_rounds": ms[f], "ms_per_step_spread": spread(ms[f]),
                        "loss_phase_ms": statistics.median(loss_ms[f]), "loss_phase_ms_rounds": loss_ms[f], "loss_phase_ms_spread": spread(loss_ms[f])}
    if len(flags) == 2:
        for key in ("ms_per_step", "loss_phase_ms"):
            diff = rec["off"][key] - rec["on"][key]
            noise = max(rec["off"][key + "_spread"], rec["on"][key + "_spread"])
            rec[key + "_off_minus_on"] = diff
            rec[key + "_verdict"] = "no gain" if abs(diff) <= noise else ("on is faster" if diff > 0 else "on is slower")
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
