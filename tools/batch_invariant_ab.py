"""Cost of batch-invariant inference (PARQDecoder.batch_invariant; include/parq_hip.h parq_set_batch_invariant): the inference forward
of bench.py's workloads with the flag off and on, at 1, 2, 4 and 8 scenes per call.

    python tools/batch_invariant_ab.py [--configs cfg3,shipped] [--scenes 1,2,4,8] [--rounds 5] [--steps 40] [--out profiles/batch_invariant_ab.json]

One process, one module per configuration.  For every scene count the two settings ALTERNATE (off, on, off, on, ...): each round switches
the flag (which drops the cached workspace and the captured graph), runs untimed forwards until the forward is replayed from its graph
again, synchronises, times `steps` forwards with the host clock and synchronises before the clock is read.  The medians over the
rounds are reported with every round's value beside them.  The record also says, per scene count, how many key splits the cross-attention
takes under either setting (the flag's main cost: the partial writes and the merge grow with them), how many graph nodes the captured
iterations have, and whether scene 0 of the batch under the flag equals that scene alone (the property that is paid for)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

KEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d", "sem_cls_prob", "coord_pos")


def ceil_div(a, b):
    return -(-a // b)


def cross_splits(B, H, Q, N, dh, cus):
    """Key splits of the default attention mode's cross-attention kernel (flash_split_pick_splits / flash_split256_pick_splits)."""
    if dh == 256:
        want = max(1, min(ceil_div(cus, B * H * ceil_div(Q, 128)), ceil_div(N, 32), 256))
        return want // 8 * 8 if want >= 8 else want
    return max(1, min(ceil_div(cus, B * H * ceil_div(Q, 256)), ceil_div(ceil_div(N, 32), 2), 256))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,shipped")
    ap.add_argument("--scenes", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from parq_amd import _lib
    assert torch.cuda.is_available(), "tools/batch_invariant_ab.py needs a GPU"
    torch.set_grad_enabled(False)
    device = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rec = {"what": "inference forward, flag off / on alternating in one process; ms per forward = host clock around `steps` forwards "
                   "between two device synchronisations, median over `rounds`",
           "rounds": a.rounds, "steps": a.steps, "gpu": torch.cuda.get_device_name(0), "compute_units": cus, "configs": {}}
    for name in a.configs.split(","):
        conf = bench.CONFIGS[name]
        bench.WORKLOAD.update({k: conf[k] for k in ("views", "image_hw", "feat_hw", "queries", "iters")})
        bench.WORKLOAD["dim"] = conf.get("dim", 256)
        h, w = bench.WORKLOAD["feat_hw"]
        V, Q, Cd, H, I = (bench.WORKLOAD[k] for k in ("views", "queries", "dim", "heads", "iters"))
        cfg, W, dec = bench.build_decoder(device)
        if conf["mode"]:
            dec.attention_mode = conf["mode"]
        rows = {}
        for B in [int(x) for x in a.scenes.split(",")]:
            inputs = bench.build_inputs(B, device, seed=1000)
            alone = tuple(t[:1].contiguous() for t in inputs)
            times, nodes = {False: [], True: []}, {}

            def settle(flag):
                dec.batch_invariant = flag
                for _ in range(a.warmup):
                    dec(*inputs, feat_hw=(h, w))
                torch.cuda.synchronize()
                entry = next(reversed(dec._ws.values()))
                assert entry.replays >= 1, "the timed forwards are meant to replay the captured graph"
                nodes[flag] = int(_lib.load().parq_graph_nodes(next(iter(entry.graphs.values()))))
            for flag in (False, True):                   # spin-up of this shape under both settings, untimed
                settle(flag)
                for _ in range(bench.PREWARM_STEPS):
                    dec(*inputs, feat_hw=(h, w))
            for rnd in range(a.rounds):
                for flag in (False, True):
                    settle(flag)
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        dec(*inputs, feat_hw=(h, w))
                    torch.cuda.synchronize()
                    times[flag].append((time.perf_counter() - t0) / a.steps * 1e3)
            # the property: scene 0 of the batch under the flag is scene 0 alone (default path)
            dec.batch_invariant = True
            got = [{k: o[k][:1].clone() for k in KEYS} for o in dec(*inputs, feat_hw=(h, w))]
            dec.batch_invariant = False
            off_b = [{k: o[k][:1].clone() for k in KEYS} for o in dec(*inputs, feat_hw=(h, w))]
            want = [{k: o[k].clone() for k in KEYS} for o in dec(*alone, feat_hw=(h, w))]
            torch.cuda.synchronize()
            same = lambda x: all(torch.equal(p[k], q[k]) for p, q in zip(x, want) for k in KEYS)
            off_ms, on_ms = statistics.median(times[False]), statistics.median(times[True])
            rows[str(B)] = {"off_ms": off_ms, "on_ms": on_ms, "on_over_off": on_ms / off_ms,
                            "off_iterations_per_s": B * I / off_ms * 1e3, "on_iterations_per_s": B * I / on_ms * 1e3,
                            "off_ms_rounds": times[False], "on_ms_rounds": times[True],
                            "cross_attention_key_splits": {"off": cross_splits(B, H, Q, V * h * w, Cd // H, cus),
                                                           "on": cross_splits(1, H, Q, V * h * w, Cd // H, cus)},
                            "graph_nodes": {"off": nodes[False], "on": nodes[True]},
                            "scene0_equals_scene0_alone": {"off": same(off_b), "on": same(got)},
                            "guard_raised": bool(dec.attention_too_peaked()), "attention_mode": dec.attention_mode}
            print(name, "B=%d" % B, json.dumps({k: rows[str(B)][k] for k in ("off_ms", "on_ms", "on_over_off", "cross_attention_key_splits",
                                                                              "graph_nodes", "scene0_equals_scene0_alone")}), flush=True)
            del inputs, alone
        rec["configs"][name] = {"workload": conf["text"], "dim": Cd, "scenes_per_call": rows}
        del dec
        torch.cuda.empty_cache()
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
