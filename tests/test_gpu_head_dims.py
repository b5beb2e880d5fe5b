"""GPU tier: head dims 32 and 128 against the float64 oracle, forward and backward.

Each head dim runs kernels of its own: at head dim 32 the one-launch self-attention, the flash cross-attention and
attn_bwd_kernel<32> (self- and cross-attention backward, dQ added with float atomics); at head dim 128 the one-launch
self-attention up to 1024 queries (flash + merge above), the flash cross-attention and the materialised backward
(attn_bwd.hip attn_bwd_materialised).  Both default to attention mode "fp32" (PARQDecoder.__init__), e.g. dim 256 with 8 heads
or dim 128 with 4.  The oracle's attention is pinned to torch's nn.MultiheadAttention arithmetic at these head dims by
tests/test_oracle_head_dims_cpu.py.

  * inference, teacher-forced: the bound and the tie masking of test_gpu_decoder.py test_ragged_shapes_vs_fp64_oracle, in the
    default mode and in mode "split" (accepted at these head dims: the attention stays fp32, and at d >= 768 the chain GEMMs
    take the fp16 x 3 tile), with the captured forward bit-identical to the uncaptured one;
  * the modes without kernels at these head dims ("fp16", "bf16", "split8") raise instead of running other arithmetic;
  * training: the bounds of test_gpu_backward.py test_backward_matches_oracle_autograd, through PARQDecoder.backward and through
    autograd + AdamW."""
import re

import numpy as np
import pytest
import torch

from parq_amd import synth
from oracle import parq_oracle as O
from gpu_util import infer, make_decoder, rel_err, scene_args, to_np
from test_gpu_backward import GKEYS, oracle_grads

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _replays(dec):
    return sum(e.replays for e in dec._ws.values())


def _forward_graph_and_direct(dec, sc):
    """The inference forward launch by launch and from a captured graph: asserts the two are bit-identical, returns the outputs."""
    args = scene_args(sc)

    def run():
        out = [{k: v.clone() for k, v in o.items()} for o in infer(dec, *args)]
        torch.cuda.synchronize()
        return out
    dec.use_graph = False
    direct = run()
    dec.use_graph = True
    n = _replays(dec)
    run()                                   # launch by launch (remembers the key)
    replayed = run()                        # captured here, and run from the graph
    assert _replays(dec) == n + 1
    for k, (a, b) in enumerate(zip(direct, replayed)):
        for key in a:
            assert torch.equal(a[key], b[key]), (k, key)
    return [to_np(o) for o in replayed]


def _worst_vs_oracle(cfg, W, sc, outs):
    """Teacher-forced float64 oracle (each iteration fed the reference points the decoder used there); asserts TOL on every output
    and returns the worst error."""
    od = O.OracleDecoder(cfg, W, synth.SCANNET_MEAN_SIZES, dtype=torch.float64)
    forced = [O.normalize(torch.from_numpy(o["coord_pos"]).double(), cfg.TRANSFORMER.SCALE) for o in outs]
    with torch.no_grad():
        want = od.forward(sc["tokens"], sc["camera"], sc["T_camera_pseudoCam"], sc["T_world_pseudoCam"],
                          sc["T_world_local"], forced_refs=forced)
    worst = 0.0
    for k, (a, b) in enumerate(zip(outs, want)):
        top2 = b["sem_cls_prob"].topk(2, -1).values
        ok = ((top2[..., 0] - top2[..., 1]) > 1e-3).numpy()
        for key in a:
            x, y = a[key], b[key].numpy()
            if key == "size_unnormalized":
                x, y = x[ok], y[ok]
            e = rel_err(x, y)
            assert e < TOL, (k, key, e)
            worst = max(worst, e)
    return worst


@pytest.mark.parametrize("B,V,h,w,Q,heads,dim,ffn", [
    # head dim 32
    (2, 3, 11, 13, 40, 8, 256, 768),       # two scenes, Q % 16 != 0
    (1, 2, 6, 5, 7, 4, 128, 96),           # fewer queries than a tile; K = 96
    (3, 1, 9, 7, 50, 2, 64, 64),           # the smallest C the library takes
    (2, 2, 23, 29, 300, 8, 256, 768),      # Q = 300: self-attention over more than 256 keys; N = 1334 ragged
    (1, 10, 30, 40, 256, 8, 256, 768),     # N = 12 000: the cross-attention splits its keys many ways (oracle: 200 MB of probabilities)
    # head dim 128
    (2, 3, 11, 13, 40, 2, 256, 768),       # two scenes, Q % 16 != 0
    (1, 2, 12, 16, 256, 4, 512, 768),      # the shipped query count, one scene
    (1, 2, 23, 29, 40, 8, 1024, 768),      # the shipped width (large-C K/V projection) with 8 heads of 128
    (1, 2, 12, 16, 256, 8, 1024, 768),     # the same with M = 256 rows: mode "split" runs the chain's fp16 x 3 tile
    (1, 1, 6, 7, 1100, 2, 256, 256),       # Q > 1024: the self-attention leaves the one-launch form for flash + merge
])
def test_inference_vs_fp64_oracle(B, V, h, w, Q, heads, dim, ffn):
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=heads, ffn=ffn, layers=3)
    W = synth.make_decoder_weights(cfg, 61)
    sc = synth.make_scene(62, B, V, h, w, dim, smooth=True)
    dec = make_decoder(cfg, W)
    assert dec.attention_mode == "fp32"
    worst, outs = {}, {}
    for mode in ("fp32", "split"):
        dec.attention_mode = mode
        outs[mode] = _forward_graph_and_direct(dec, sc)
        worst[mode] = _worst_vs_oracle(cfg, W, sc, outs[mode])
    print("\nhead dim %d, worst error against float64 (bound %.0e):" % (dim // heads, TOL), worst)
    # mode "split" keeps the fp32 attention here (no split cache at these head dims); what it changes is the chain's GEMMs that contract
    # over 768 / 1024 (the fp16 x 3 tile: api.hip build_derived_weights, d >= 768), on row counts in multiples of 16 (chain.hip)
    if dim >= 768 and (B * Q) % 16 == 0:
        assert any(not np.array_equal(a[k], b[k]) for a, b in zip(outs["fp32"], outs["split"]) for k in a)


@pytest.mark.parametrize("dim,heads", [(256, 8), (256, 2)])
@pytest.mark.parametrize("mode", ["fp16", "bf16", "split8"])
def test_modes_without_kernels_at_this_head_dim_raise(mode, dim, heads):
    cfg = synth.decoder_cfg(dim=dim, queries=16, heads=heads, ffn=64, layers=2)
    dec = make_decoder(cfg, synth.make_decoder_weights(cfg, 63))
    sc = synth.make_scene(64, 1, 1, 5, 6, dim, smooth=True)
    want = [{k: v.clone() for k, v in o.items()} for o in infer(dec, *scene_args(sc))]
    dec.attention_mode = mode
    msg = "attention mode 4 needs a head dim of 64" if mode == "split8" else "the fp16 / bf16 attention modes need head dim 64"
    with pytest.raises(RuntimeError, match="parq_set_attention_mode failed .*" + re.escape(msg)):
        infer(dec, *scene_args(sc))
    dec.attention_mode = "fp32"                 # the handle is still usable, in the mode it had
    got = infer(dec, *scene_args(sc))
    torch.cuda.synchronize()
    assert all(torch.equal(a[k], b[k]) for a, b in zip(want, got) for k in a)


def _scene_and_cotangents(B, V, h, w, Q, dim, cfg, layers):
    sc = synth.make_scene(72, B, V, h, w, dim, smooth=True)
    ncls = cfg.NUM_SEMCLS + 1
    cots = {"pred_logits": synth.normal(73, "cl", (layers, B, Q, ncls)), "center_unnormalized": synth.normal(74, "cc", (layers, B, Q, 3)),
            "size_unnormalized": synth.normal(75, "cs", (layers, B, Q, 3)), "ortho6d": synth.normal(76, "cr", (layers, B, Q, 6))}
    return sc, cots


def _grad_err(got, ref):
    """(Frobenius-relative, max-relative) error of a gradient against its float64 reference."""
    d = got.astype(np.float64) - ref
    return np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-9), np.abs(d).max() / max(np.abs(ref).max(), 1e-9)


@pytest.mark.parametrize("B,V,h,w,Q,heads,dim,ffn,layers,shared", [
    # head dim 32: attn_bwd_kernel<32> (256 keys per workgroup, queries in tiles of 32, dQ by float atomics)
    (2, 2, 8, 10, 32, 8, 256, 96, 2, True),       # N = 160: one partial workgroup of keys
    (1, 3, 6, 7, 40, 4, 128, 128, 3, True),       # Q = 40: a query-tile tail of 8
    (2, 2, 32, 41, 24, 8, 256, 128, 3, True),     # N = 2624: 11 key workgroups adding into dQ; shared layers: every iteration's launch adds
                                                  # into the same dK / dV (accumulate_kv)
    (1, 2, 10, 13, 20, 8, 256, 96, 2, False),     # unshared layers, N = 260
    (1, 2, 9, 11, 300, 8, 256, 96, 2, True),      # self-attention backward over two key workgroups (the second holds 44 keys), 10 query tiles
    (2, 1, 5, 6, 16, 2, 64, 64, 2, True),         # the smallest C
    # head dim 128: the materialised backward
    (2, 2, 32, 41, 24, 2, 256, 128, 3, True),     # N = 2624, accumulating over the iterations (a ReLU input of 1.7e-7 in the heads flips its
                                                  # mask between fp32 and float64 here: ~3e-4 Frobenius, 100x the other rows, inside the bounds)
    (1, 2, 12, 16, 40, 4, 512, 256, 2, False),    # unshared layers, d = 512
])
def test_backward_matches_oracle_autograd(B, V, h, w, Q, heads, dim, ffn, layers, shared):
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=heads, ffn=ffn, layers=layers, share_weights=shared, dropout=0.0)
    W = synth.make_decoder_weights(cfg, 71, damped=True)        # free-running over the iterations: the damped centre head
    sc, cots = _scene_and_cotangents(B, V, h, w, Q, dim, cfg, layers)
    want, want_tok, oouts = oracle_grads(cfg, W, sc, cots)

    dec = make_decoder(cfg, W)
    assert dec.attention_mode == "fp32" and dec._train_mode() == "fp32"
    outs = dec.forward_train(*scene_args(sc))
    ferr = 0.0
    for k in range(layers):
        for key in GKEYS:
            a, b = outs[k][key].cpu().numpy(), oouts[k][key].detach().numpy()
            e = np.abs(a - b).max() / max(1.0, np.abs(b).max())
            assert e < 1e-4, (k, key, e)
            ferr = max(ferr, e)
    grads, d_tok = dec.backward({k: torch.from_numpy(v) for k, v in cots.items()})
    worst = {}
    for name, g in grads.items():
        if name not in want:
            assert float(g.abs().max()) == 0.0, name
            continue
        worst[name] = _grad_err(g.cpu().numpy(), want[name].numpy())
    terr = _grad_err(d_tok.cpu().numpy(), want_tok.numpy())
    print("\nhead dim %d: training forward %.3e (bound 1e-4); gradients (frobenius, max; bounds 2e-3, 2e-2): worst frobenius %s, "
          "worst max %s, tokens %.3e %.3e" % (dim // heads, ferr, max(worst.items(), key=lambda kv: kv[1][0]),
                                               max(worst.items(), key=lambda kv: kv[1][1]), *terr))
    bad = {k: v for k, v in worst.items() if not (v[0] < 2e-3 and v[1] < 2e-2)}
    assert not bad, bad
    assert terr[0] < 2e-3 and terr[1] < 2e-2, terr


def test_autograd_node_and_adamw_steps_at_head_dim_32():
    """test_gpu_backward.py test_autograd_node_and_adamw_steps with 4 heads of 32: loss.backward() fills .grad of the parameters and
    of the tokens within the bounds above, and a few AdamW steps lower a regression loss."""
    B, V, h, w, Q, dim, layers = 2, 2, 8, 10, 32, 128, 2
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=4, ffn=96, layers=layers, dropout=0.0)
    W = synth.make_decoder_weights(cfg, 81, damped=True)
    sc, cots = _scene_and_cotangents(B, V, h, w, Q, dim, cfg, layers)
    dec = make_decoder(cfg, W).train()
    assert dec.attention_mode == "fp32"
    args = list(scene_args(sc))
    args[0] = args[0].clone().requires_grad_(True)
    outs = dec(*args)
    loss = sum((outs[k][key] * torch.from_numpy(cots[key][k]).cuda()).sum() for k in range(layers) for key in GKEYS)
    loss.backward()
    want, want_tok, _ = oracle_grads(cfg, W, sc, cots)
    seen = 0
    for name, p in dec.named_parameters():
        if name in want and p.grad is not None:
            err = _grad_err(p.grad.cpu().numpy(), want[name].numpy())
            assert err[0] < 2e-3 and err[1] < 2e-2, (name, err)
            seen += 1
    assert seen >= 30
    err = _grad_err(args[0].grad.cpu().numpy(), want_tok.numpy())
    assert err[0] < 2e-3 and err[1] < 2e-2, err

    opt = torch.optim.AdamW([p for p in dec.parameters() if p.requires_grad], lr=2e-3, weight_decay=1e-4)
    target = torch.from_numpy(synth.uniform(90, "tgt", (B, Q, 3), -1.0, 1.0)).cuda()
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        outs = dec(*scene_args(sc))
        l = sum(((o["center_unnormalized"] - target) ** 2).mean() for o in outs)
        l.backward()
        torch.nn.utils.clip_grad_norm_(dec.parameters(), 1.0)
        opt.step()
        losses.append(float(l))
    print("\nregression loss over AdamW steps at head dim 32:", ["%.4f" % x for x in losses])
    assert losses[-1] < losses[0]
