"""Generate the golden vectors under tests/golden from the REAL reference.

DEV-CONTAINER ONLY (needs /root/reference).  Run:  python -m oracle.make_golden

For every case the real ``PARQDecoder`` / ``AddRayPE`` is imported in place
(oracle/reference_loader.py), loaded with the seeded synthetic weights of
``parq_amd/synth.py`` and run on the seeded synthetic scene; only the OUTPUTS
(plus the case description needed to regenerate the inputs, and decision
margins) are written.  No reference source or bytecode is stored.

Cases:
  g1_cfg1        BASELINE cfg 1: 2 views 60x80, Q=64, I=1, d=256, noise features
  g2_forced      B=2, 4 views 60x80, Q=64, I=8, d=256, noise features — consumed
                 teacher-forced: iteration k is fed norm(coord_pos_k)
  g3_damped      B=1, 4 views 60x80, Q=64, I=8, smooth features, centre head x0.05 —
                 consumed free-running
  g4_edges       hand-placed reference points (behind camera, partial texels,
                 all views invalid, clamp limits), ragged Q=40, N=429, d=128/H=2
  g5_raype       AddRayPE on a 2-view 6x8 grid, C=64
  g6_shipped     shipped dims d=1024/H=4 (head dim 256), FFN 768, 2 views 15x20, Q=32, I=2
  g7_fp64        the g2 case run by the reference in float64
  g8_unshared    SHARE_WEIGHTS=False, 2 layers, d=128/H=2
  g14_cfg3       BASELINE cfg 3 exactly (the benchmark's headline size): 10 views 120x160 feature maps
                 (N = 192 000 tokens), Q=256, I=8, d=256, noise features — consumed teacher-forced
  g15_cfg5_shape BASELINE cfg 5's decoder shape on small feature maps: 20 views 24x32 (N = 15 360 tokens), Q=512 (two
                 query tiles per head), I=12, d=256, noise features — consumed teacher-forced (split and fp16 modes)
  g16_module     the MODULE-level composition, captured through the reference's own PARQ.forward
                 (model/parq_lightning.py:68-95: backbone hand-off -> AddRayPE -> features + encoding -> tokenisation ->
                 decoder) with a stub backbone that returns seeded features: per-iteration output dicts of the free-running
                 (damped) decoder plus a float64 checksum of the token tensor
  g17_grads      GRADIENTS of the reference's own autograd (float64, eval mode = dropout off, as the reference differentiates
                 in eval mode too): two small damped cases (d=128/2 heads and d=256/4 heads, 2 scenes, 3 free-running
                 iterations), each under (i) a linear cotangent loss sum_k <c_k, out_k> and (ii) the reference's own
                 PARQDecoder.loss (Hungarian matcher, np.random.seed fixed) -> .backward(); per-parameter gradients (whole
                 tensors up to 8192 elements, else norm + sum + strided sample), a strided sample of d tokens, and the names of
                 the parameters the reference leaves without gradient.  Pins detach placement (transformer_parq.py:331-332),
                 the no-grad probabilities (:261-265), the arg-max size gather (utils/parq_utils.py:96-98) and the loss
  g20_raype_grads gradients of the reference's AddRayPE under its own autograd (float64): tokens = features + encoding, tokenised as
                 model/parq_lightning.py:72-85 does, loss = <cotangent, tokens>; d encoder.{0,2}.{weight,bias} and d features
  g18_cfg3_smooth BASELINE cfg 3's geometry (10 views 120x160, Q=256, I=8, d=256) on SMOOTH (FPN-like) features, where the
                 reference's fp32 run stays within ~6e-5 of its float64 evaluation: consumed teacher-forced at an UNRELAXED 1e-4
  g19_cfg2       BASELINE cfg 2's exact geometry: 5 views 120x160 (N = 96 000), Q=128, I=4, d=256, smooth features
                 (teacher-forced: split mode at an unrelaxed 1e-4, bf16 / fp16 modes at their stated bounds)
  g21_peaked     PEAKED cross-attention: cfg 2's geometry with the query rows of the cross-attention in-projection
                 (transformer_parq.py:377-380) scaled by 4, so that rows rest on a handful of keys (row probability sums down to ~1:
                 the regime trained detectors attend in) — consumed teacher-forced at an unrelaxed 1e-4 in whatever
                 tier the peakedness guard of attention mode "split8" selects (the guard has to trip on it)
  g22_reference_ops the reference's free-running fp32 outputs (all iterations) at the three shapes of
                 tests/test_oracle_vs_reference.py (weights seed 901, scene seed 902): what the oracle's reference_ops
                 mode, bench.py's cpu_baseline, is held to without the reference tree
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from parq_amd import synth                      # noqa: E402
from oracle import reference_loader as RL        # noqa: E402
from oracle import parq_oracle as O              # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden")
KEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d", "sem_cls_prob", "coord_pos")

CASES = {
    "g1_cfg1": dict(cfg=dict(dim=256, queries=64, heads=4, ffn=768, layers=1), wseed=11, sseed=101,
                    B=1, V=2, h=60, w=80, smooth=False, damped=False),
    "g2_forced": dict(cfg=dict(dim=256, queries=64, heads=4, ffn=768, layers=8), wseed=12, sseed=102,
                      B=2, V=4, h=60, w=80, smooth=False, damped=False),
    "g3_damped": dict(cfg=dict(dim=256, queries=64, heads=4, ffn=768, layers=8), wseed=13, sseed=103,
                      B=1, V=4, h=60, w=80, smooth=True, damped=True),
    "g4_edges": dict(cfg=dict(dim=128, queries=40, heads=2, ffn=96, layers=2,
                              scale=[-3.0, 3.0, -2.0, 0.5, -1.0, 5.25]), wseed=14, sseed=104,
                     B=2, V=3, h=11, w=13, smooth=False, damped=False, edges=True),
    "g6_shipped": dict(cfg=dict(dim=1024, queries=32, heads=4, ffn=768, layers=2), wseed=16, sseed=106,
                       B=1, V=2, h=15, w=20, smooth=False, damped=False),
    "g7_fp64": dict(cfg=dict(dim=256, queries=64, heads=4, ffn=768, layers=8), wseed=12, sseed=102,
                    B=2, V=4, h=60, w=80, smooth=False, damped=False, double=True),
    "g8_unshared": dict(cfg=dict(dim=128, queries=32, heads=2, ffn=192, layers=2, share_weights=False),
                        wseed=18, sseed=108, B=1, V=2, h=12, w=16, smooth=False, damped=False),
    "g14_cfg3": dict(cfg=dict(dim=256, queries=256, heads=4, ffn=768, layers=8), wseed=24, sseed=124,
                     B=1, V=10, h=120, w=160, smooth=False, damped=False),
    "g15_cfg5_shape": dict(cfg=dict(dim=256, queries=512, heads=4, ffn=768, layers=12), wseed=25, sseed=125,
                           B=1, V=20, h=24, w=32, smooth=False, damped=False),
    # g18 / g19 are consumed at an UNRELAXED 1e-4 against the reference's fp32 vectors.  That is only meaningful where the
    # reference's own fp32 run is well inside 1e-4 of its float64 evaluation; on undamped weights that deviation varies with the
    # seed between 1e-5 and 2e-4 even on smooth features (profiles/r04_reference_self_noise_scan.txt: 4 seed pairs scanned for
    # g18, 7 for g19, with this file's own run_reference + the float64 oracle).  The pairs below are the scanned ones with the
    # smallest deviation (6.6e-5 / 1.0e-5); the rejected ones are listed in that file.
    "g18_cfg3_smooth": dict(cfg=dict(dim=256, queries=256, heads=4, ffn=768, layers=8), wseed=38, sseed=138,
                            B=1, V=10, h=120, w=160, smooth=True, damped=False),
    "g19_cfg2": dict(cfg=dict(dim=256, queries=128, heads=4, ffn=768, layers=4), wseed=31, sseed=131,
                     B=1, V=5, h=120, w=160, smooth=True, damped=False),
    # seeds from the same kind of scan (profiles/r05_reference_self_noise_scan_peaked.txt, oracle/make_golden.py scan ...)
    "g21_peaked": dict(cfg=dict(dim=256, queries=128, heads=4, ffn=768, layers=4), wseed=53, sseed=153,
                       B=1, V=5, h=120, w=160, smooth=True, damped=False, wq_scale=4.0),
}

# gradient cases (g17): the reference's own autograd in float64, eval mode, free-running on damped weights / smooth features
GRAD_CASES = {
    "d128": dict(cfg=dict(dim=128, queries=24, heads=2, ffn=96, layers=3), wseed=41, sseed=141, cseed=241, bseed=341,
                 B=2, V=3, h=10, w=12, nbox=4, max_box=8, np_seed=777),
    "d256": dict(cfg=dict(dim=256, queries=32, heads=4, ffn=256, layers=3), wseed=42, sseed=142, cseed=242, bseed=342,
                 B=2, V=2, h=12, w=16, nbox=5, max_box=8, np_seed=778),
}
GRAD_KEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d")
GRAD_FULL_MAX = 8192          # tensors up to this many elements are stored whole
GRAD_STRIDE = 53              # larger ones: norm, sum and every 53rd element of the flattened tensor
TOKEN_STRIDE = 17


def grad_case_inputs(c):
    """(cfg, weights, scene, cotangents, padded boxes, symmetry classes) of a gradient case — shared with the tests."""
    cfg = synth.decoder_cfg(**c["cfg"])
    W = synth.make_decoder_weights(cfg, c["wseed"], damped=True)
    sc = synth.make_scene(c["sseed"], c["B"], c["V"], c["h"], c["w"], cfg.DIM_IN, smooth=True)
    I, B, Q, ncls = cfg.TRANSFORMER.DEC_LAYERS, c["B"], cfg.NUM_QUERIES, cfg.NUM_SEMCLS + 1
    cots = {k: synth.normal(c["cseed"] + i, "cot." + k, (I, B, Q, wd))
            for i, (k, wd) in enumerate(zip(GRAD_KEYS, (ncls, 3, 3, 6)))}
    obbs, sym = synth.make_boxes(c["bseed"], B, c["nbox"], max_box=c["max_box"])
    return cfg, W, sc, cots, obbs, sym


def grad_summary(g):
    """What the fixture keeps of one gradient tensor (float64)."""
    g = np.asarray(g, np.float64).reshape(-1)
    if g.size <= GRAD_FULL_MAX:
        return {"full": g}
    return {"norm": np.array([np.linalg.norm(g), g.sum()]), "sample": g[::GRAD_STRIDE].copy()}


RAYPE_GRAD_CASE = dict(dim=256, seed=91, gseed=92, fseed=93, cseed=94, B=2, V=3, h=7, w=9,
                       ray_points_scale=[-3.0, 3.0, -2.0, 0.5, 0.25, 5.25])


def raype_grad_case_inputs(c):
    Wp = synth.make_ray_pe_weights(c["dim"], c["seed"])
    geom = synth.make_geometry(c["gseed"], c["B"], c["V"], c["h"], c["w"])
    feat = synth.normal(c["fseed"], "feat", (c["B"], c["V"], c["dim"], c["h"], c["w"]))
    cot = synth.normal(c["cseed"], "cot", (c["B"], c["V"] * c["h"] * c["w"], c["dim"]))
    return Wp, geom, feat, cot


def make_raype_grad_golden(ref):
    """g20: the reference's AddRayPE (model/ray_positional_encoding.py:61-139) in float64 under its own autograd, composed as
    PARQ.forward composes it (model/parq_lightning.py:72-85: images_feat = features + encoding, then 'b t c h w -> b (t h w) c')."""
    from einops import rearrange
    c = RAYPE_GRAD_CASE
    Wp, (cam, T_cp, T_wp, T_wl), feat, cot = raype_grad_case_inputs(c)
    pe = ref.AddRayPE(c["dim"], c["ray_points_scale"], 64, 0.25, 5.25).double()
    pe.load_state_dict({k: torch.from_numpy(v).double() for k, v in Wp.items()}, strict=True)
    f = torch.from_numpy(feat).double().requires_grad_(True)
    dbl = lambda a: torch.from_numpy(a).double()
    enc = pe(f, ref.Camera(dbl(cam)), ref.Pose(dbl(T_cp)), ref.Pose(dbl(T_wp)), ref.Pose(dbl(T_wl)))
    tokens = rearrange(f + enc, "b t c h w -> b (t h w) c")
    loss = (tokens * dbl(cot)).sum()
    loss.backward()
    arrays = {"loss_value": np.float64(float(loss.detach())), "tokens_sample": tokens.detach().numpy()[:, ::11, ::7].copy()}
    for name, p in pe.named_parameters():
        for k, v in grad_summary(p.grad.numpy()).items():
            arrays["grad/%s/%s" % (name, k)] = v
    fg = f.grad.numpy().reshape(-1)
    arrays["dfeat/norm"] = np.array([np.linalg.norm(fg), fg.sum()])
    arrays["dfeat/sample"] = fg[::TOKEN_STRIDE].copy()
    arrays["meta"] = np.frombuffer(json.dumps(c, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT_DIR, "g20_raype_grads.npz"), **arrays)
    print("wrote g20_raype_grads: loss %.6f, %d arrays" % (float(loss.detach()), len(arrays)))


def make_grad_golden(ref):
    """g17: gradients of the imported reference (model/parq_lightning.py:97-100 differentiates losses['total_loss'];
    model/parq_decoder.py:264-370 the loss; model/transformer_parq.py:331-332 detach between iterations)."""
    arrays, meta = {}, {}
    for tag, c in GRAD_CASES.items():
        cfg, W, sc, cots, obbs, sym = grad_case_inputs(c)
        for kind in ("linear", "setloss"):
            dec = RL.build_reference_decoder(ref, cfg, W, double=True)          # eval mode: dropout off, autograd on
            tokens = torch.from_numpy(sc["tokens"]).double().requires_grad_(True)
            outs = dec(tokens, ref.Camera(torch.from_numpy(sc["camera"]).double()),
                       ref.Pose(torch.from_numpy(sc["T_camera_pseudoCam"]).double()),
                       ref.Pose(torch.from_numpy(sc["T_world_pseudoCam"]).double()),
                       ref.Pose(torch.from_numpy(sc["T_world_local"]).double()))
            if kind == "linear":
                loss = sum((o[k] * torch.from_numpy(cots[k][i]).double()).sum() for i, o in enumerate(outs) for k in GRAD_KEYS)
            else:
                np.random.seed(c["np_seed"])
                # the reference builds its y-rotation tables with torch.tensor(...) in the DEFAULT dtype (parq_decoder.py:205-262):
                # float64 as the default makes its loss run in float64 end to end
                torch.set_default_dtype(torch.float64)
                dec.class_weight = dec.class_weight.double()          # a plain tensor attribute (parq_decoder.py:46-48): .double() skips it
                try:
                    ld = dec.loss(outs, ref.Obb3D(torch.from_numpy(obbs).double()),
                                  ref.Pose(torch.from_numpy(sc["T_world_local"]).double()), torch.from_numpy(sym).double())
                finally:
                    torch.set_default_dtype(torch.float32)
                loss = ld["total_loss"]
                for k, v in ld.items():
                    arrays["%s/%s/loss/%s" % (tag, kind, k)] = np.float64(float(v))
            loss.backward()
            arrays["%s/%s/loss_value" % (tag, kind)] = np.float64(float(loss))
            nograd = []
            seen = set()
            for name, p in dec.named_parameters():                # remove_duplicate: the shared heads appear once (mlp_heads.*)
                if id(p) in seen:
                    continue
                seen.add(id(p))
                if p.grad is None:
                    nograd.append(name)
                    continue
                for k, v in grad_summary(p.grad.numpy()).items():
                    arrays["%s/%s/grad/%s/%s" % (tag, kind, name, k)] = v
            tg = tokens.grad.numpy().reshape(-1)
            arrays["%s/%s/dtokens/norm" % (tag, kind)] = np.array([np.linalg.norm(tg), tg.sum()])
            arrays["%s/%s/dtokens/sample" % (tag, kind)] = tg[::TOKEN_STRIDE].copy()
            for i, o in enumerate(outs):                          # the free-running forward outputs, for the forward half of the test
                for k in KEYS:
                    arrays["%s/%s/out/it%d_%s" % (tag, kind, i, k)] = o[k].detach().numpy()
            meta["%s/%s/nograd" % (tag, kind)] = nograd
            print("g17 %s %-8s loss %.6f  params with grad %d, without %s" % (tag, kind, float(loss), len(seen) - len(nograd), nograd))
    meta["cases"] = GRAD_CASES
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT_DIR, "g17_grads.npz"), **arrays)
    print("wrote g17_grads", len(arrays), "arrays")

# module-level case (g16): PARQ.forward = stub backbone -> AddRayPE -> tokenise -> decoder, free-running on damped weights
MODULE_CASE = dict(cfg=dict(dim=256, queries=48, heads=4, ffn=768, layers=4), wseed=26, pseed=27, gseed=126, fseed=127,
                   B=2, V=3, h=14, w=18, feat_std=0.5, ray_points_scale=[-3.0, 3.0, -2.0, 0.5, 0.25, 5.25])


def module_case_inputs(c):
    """(decoder cfg, decoder weights, ray-PE weights, geometry, features) of the module-level case — shared with the tests."""
    cfg = synth.decoder_cfg(**c["cfg"])
    W = synth.make_decoder_weights(cfg, c["wseed"], damped=True)
    Wp = synth.make_ray_pe_weights(c["cfg"]["dim"], c["pseed"])
    geom = synth.make_geometry(c["gseed"], c["B"], c["V"], c["h"], c["w"])
    feat = synth.normal(c["fseed"], "feat", (c["B"], c["V"], c["cfg"]["dim"], c["h"], c["w"]), std=c["feat_std"])
    return cfg, W, Wp, geom, feat


def make_module_golden(ref):
    """g16: run the reference's own PARQ.forward (model/parq_lightning.py:68-95).  The Lightning module is built without its
    constructor (which downloads a torchvision ResNet): `backbone2d` is a stub that hands over seeded feature maps the way
    ResnetFPN.forward does (batch['all_features']), `add_ray_pe` and `box3d_decoder` are the reference's real modules."""
    from model import parq_lightning as PL              # noqa: E402  (reference module, imported in place)
    c = MODULE_CASE
    cfg, W, Wp, (cam, T_cp, T_wp, T_wl), feat = module_case_inputs(c)
    model = PL.PARQ.__new__(PL.PARQ)
    torch.nn.Module.__init__(model)

    class StubBackbone(torch.nn.Module):
        def forward(self, batch):
            batch["all_features"] = torch.from_numpy(feat)
            return batch

    model.backbone2d = StubBackbone()
    model.add_ray_pe = ref.AddRayPE(c["cfg"]["dim"], c["ray_points_scale"], 64, 0.25, 5.25)
    model.add_ray_pe.load_state_dict({k: torch.from_numpy(v) for k, v in Wp.items()}, strict=True)
    model.box3d_decoder = RL.build_reference_decoder(ref, cfg, W)
    model.eval()
    captured = {}
    real_dec_forward = model.box3d_decoder.forward

    def spy(tokens, *a, **k):                           # the token tensor the reference hands to its decoder
        captured["tokens"] = tokens.detach().clone()
        return real_dec_forward(tokens, *a, **k)

    model.box3d_decoder.forward = spy
    batch = {"camera_feature": ref.Camera(torch.from_numpy(cam)), "T_camera_pseudoCam": ref.Pose(torch.from_numpy(T_cp)),
             "T_world_pseudoCam": ref.Pose(torch.from_numpy(T_wp)), "T_world_local": ref.Pose(torch.from_numpy(T_wl))}
    with torch.no_grad():
        losses, outs = PL.PARQ.forward(model, batch, 0)
    assert losses == {"total_loss": 0}
    tok = captured["tokens"]
    arrays = {}
    for k, o in enumerate(outs):
        for key in KEYS:
            arrays["it%d_%s" % (k, key)] = o[key].detach().numpy().astype(np.float32)
    sc = dict(tokens=tok.numpy(), camera=cam, T_camera_pseudoCam=T_cp, T_world_pseudoCam=T_wp, T_world_local=T_wl)
    arrays.update(margins(cfg, W, sc, outs))
    # the token tensor itself is 2 x 756 x 256 floats: stored as checksums plus a strided sample
    arrays["tokens_sum"] = np.array([tok.double().sum().item(), tok.double().abs().sum().item(), (tok.double() ** 2).sum().item()])
    arrays["tokens_sample"] = tok.numpy()[:, ::37, ::5].copy()
    arrays["meta"] = np.frombuffer(json.dumps(c, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT_DIR, "g16_module.npz"), **arrays)
    print("wrote g16_module", tuple(tok.shape), len(outs))


RAYPE_CASE = dict(dim=64, seed=15, sseed=105, B=1, V=2, h=6, w=8,
                  ray_points_scale=[-3.0, 3.0, -2.0, 0.5, 0.25, 5.25])
# d = 256: the dimension of the BASELINE configurations (the library's fused ray-PE path); 2 scenes x 3 views of
# 7 x 9 pixels = 378 tokens, so the 64-token tiles straddle views and scenes and the last one is partial
RAYPE_CASE_D256 = dict(dim=256, seed=16, sseed=106, B=2, V=3, h=7, w=9,
                       ray_points_scale=[-3.0, 3.0, -2.0, 0.5, 0.25, 5.25])


def case_inputs(case):
    """(cfg, weights, scene) of a golden case — shared with the tests."""
    cfg = synth.decoder_cfg(**case["cfg"])
    W = synth.make_decoder_weights(cfg, case["wseed"], damped=case.get("damped", False))
    sc = synth.make_scene(case["sseed"], case["B"], case["V"], case["h"], case["w"], cfg.DIM_IN,
                          smooth=case.get("smooth", False))
    if case.get("edges"):
        W["refpoint.weight"] = edge_refpoints(cfg, sc, case)
    if case.get("wq_scale"):
        # sharpened cross-attention: the QUERY rows of every layer's in-projection (weight and bias) times wq_scale
        C = cfg.DIM_IN
        for k in list(W):
            if k.endswith("multihead_attn.in_proj_weight") or k.endswith("multihead_attn.in_proj_bias"):
                w = W[k].copy()
                w[:C] *= np.float32(case["wq_scale"])
                W[k] = w
    return cfg, W, sc


def edge_refpoints(cfg, sc, case):
    """Hand-placed reference points for g4 (SURVEY.md Appendix B traps 1-3, 6).

    View 0 of scene 0 is given an identity camera<-local transform by making all
    three poses of that view identity-compatible, so pixel coordinates of the
    hand-placed points are known in closed form there.
    """
    Q = cfg.NUM_QUERIES
    scale = cfg.TRANSFORMER.SCALE
    lo = np.array(scale[0::2])
    hi = np.array(scale[1::2])
    # make T_camera_local(view 0, every scene) = identity: T_cp = I, T_wp = T_wl
    sc["T_camera_pseudoCam"][:, 0] = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    sc["T_world_pseudoCam"][:, 0] = sc["T_world_local"][:, 0]
    w, h, fx, fy, cx, cy = [float(x) for x in sc["camera"][0, 0]]
    rng = synth.uniform(case["wseed"], "edge.base", (Q, 3), 0.05, 0.95).astype(np.float64)
    P = rng * (hi - lo) + lo

    def at_pixel(u, v, z):
        return np.array([(u - cx) * z / fx, (v - cy) * z / fy, z])
    P[0] = at_pixel(-0.5, 3.3, 2.0)            # partial texel left of the image: invalid but sampled
    P[1] = at_pixel(w - 0.5, 4.2, 2.0)         # partial texel right of the image
    P[2] = at_pixel(5.5, -0.75, 1.5)           # partial texel above
    P[3] = at_pixel(6.25, h - 0.25, 1.5)       # partial texel below
    # just inside the closed corners (exactly ON the corner the valid flag is a coin toss
    # under fp32 rounding, and GroupNorm spreads one flipped query over the whole scene)
    P[4] = at_pixel(0.125, 0.125, 1.0)
    P[5] = at_pixel(w - 1.125, h - 1.125, 1.0)
    P[6] = np.array([0.3, -0.4, -0.5])         # behind the camera (z < 0)
    P[7] = np.array([0.2, -0.1, 5e-4])         # z below the 1e-3 front threshold
    P[8] = np.array([2.9, -1.9, 0.3])          # far outside every view
    P[9] = at_pixel(3.0, 2.0, 4.0)             # exact texel centre
    r = (P - lo) / (hi - lo)
    wgt = np.log(np.clip(r, 1e-9, 1 - 1e-9) / (1 - np.clip(r, 1e-9, 1 - 1e-9)))
    wgt[10] = [20.0, -20.0, 0.0]               # sigmoid saturates: isig clamp limits (eps=1e-3)
    wgt[11] = [-20.0, 20.0, 20.0]
    wgt[12] = [7.5, -7.5, 0.0]                 # within 1e-3 of 0/1: clamped centre update
    return wgt.astype(np.float32)


def run_reference(ref, case):
    cfg, W, sc = case_inputs(case)
    double = case.get("double", False)
    dec = RL.build_reference_decoder(ref, cfg, W, double=double)
    cast = (lambda a: torch.from_numpy(a).double()) if double else torch.from_numpy
    with torch.no_grad():
        outs = dec(cast(sc["tokens"]), ref.Camera(cast(sc["camera"])),
                   ref.Pose(cast(sc["T_camera_pseudoCam"])), ref.Pose(cast(sc["T_world_pseudoCam"])),
                   ref.Pose(cast(sc["T_world_local"])))
    return cfg, W, sc, outs


def margins(cfg, W, sc, outs):
    """Decision margins per iteration (float64 oracle at the reference's own
    reference points): top-2 class-probability gap and the distance of every
    projected point to the closed validity boundary [0,size-1] / z=1e-3."""
    od = O.OracleDecoder(cfg, W, synth.SCANNET_MEAN_SIZES, dtype=torch.float64)
    od.prepare(sc["tokens"], sc["camera"], sc["T_camera_pseudoCam"], sc["T_world_pseudoCam"],
               sc["T_world_local"])
    res = {}
    for k, o in enumerate(outs):
        ref_k = O.normalize(o["coord_pos"].double(), cfg.TRANSFORMER.SCALE)
        pc = O.pose_transform(od.T_cl, O.denormalize(ref_k, cfg.TRANSFORMER.SCALE).unsqueeze(1))
        p2d, _ = O.camera_project(od.cam, pc)
        size = od.cam[..., :2].unsqueeze(-2)
        d = torch.minimum(p2d.abs(), (p2d - (size - 1)).abs()).min(-1).values      # (B,V,Q)
        d = torch.minimum(d, (pc[..., 2] - 1e-3).abs())
        top2 = o["sem_cls_prob"].double().topk(2, -1).values
        res["it%d_valid_margin" % k] = d.min(1).values.float().numpy()              # (B,Q)
        res["it%d_cls_margin" % k] = (top2[..., 0] - top2[..., 1]).float().numpy()
    return res


def main(only=None):
    ref = RL.load()
    os.makedirs(OUT_DIR, exist_ok=True)
    for name, case in CASES.items():
        if only and name not in only:
            continue
        cfg, W, sc, outs = run_reference(ref, case)
        arrays = {}
        for k, o in enumerate(outs):
            for key in KEYS:
                a = o[key].detach().numpy()
                arrays["it%d_%s" % (k, key)] = a.astype(np.float64 if case.get("double") else np.float32)
        arrays.update(margins(cfg, W, sc, outs))
        arrays["meta"] = np.frombuffer(json.dumps(case, sort_keys=True).encode(), dtype=np.uint8)
        np.savez_compressed(os.path.join(OUT_DIR, name + ".npz"), **arrays)
        print("wrote", name, {k: v.shape for k, v in list(arrays.items())[:3]})
    if not only or "state_dict_keys" in only:
        # schema of the reference module's state_dict (names + shapes only) for the drop-in check
        schema = {}
        for tag, kw in (("shared_d256", dict(dim=256, queries=64, heads=4, ffn=768, layers=8)),
                        ("unshared_d128", dict(dim=128, queries=32, heads=2, ffn=192, layers=2, share_weights=False))):
            cfg = synth.decoder_cfg(**kw)
            cfg.MEAN_SIZE_PATH = ref.mean_size_path
            sd = ref.PARQDecoder(cfg).state_dict()
            schema[tag] = {"cfg": kw, "keys": {k: list(v.shape) for k, v in sd.items()}}
        with open(os.path.join(OUT_DIR, "state_dict_keys.json"), "w") as f:
            json.dump(schema, f, indent=1, sort_keys=True)
        print("wrote state_dict_keys.json")
    for gname, c in (("g5_raype", RAYPE_CASE), ("g9_raype_d256", RAYPE_CASE_D256)):
        if only and gname not in only:
            continue
        Wp = synth.make_ray_pe_weights(c["dim"], c["seed"])
        cam, T_cp, T_wp, T_wl = synth.make_geometry(c["sseed"], c["B"], c["V"], c["h"], c["w"])
        pe = ref.AddRayPE(c["dim"], c["ray_points_scale"], 64, 0.25, 5.25).eval()
        pe.load_state_dict({k: torch.from_numpy(v) for k, v in Wp.items()}, strict=True)
        feat = torch.zeros(c["B"], c["V"], c["dim"], c["h"], c["w"])
        with torch.no_grad():
            enc = pe(feat, ref.Camera(torch.from_numpy(cam)), ref.Pose(torch.from_numpy(T_cp)),
                     ref.Pose(torch.from_numpy(T_wp)), ref.Pose(torch.from_numpy(T_wl)))
        np.savez_compressed(os.path.join(OUT_DIR, gname + ".npz"), encoding=enc.numpy(),
                            meta=np.frombuffer(json.dumps(c, sort_keys=True).encode(), dtype=np.uint8))
        print("wrote", gname, tuple(enc.shape))
    if not only or "g16_module" in only:
        make_module_golden(ref)
    if not only or "g17_grads" in only:
        make_grad_golden(ref)
    if not only or "g20_raype_grads" in only:
        make_raype_grad_golden(ref)
    if not only or "g10_loss" in only:
        make_loss_golden(ref)
    if not only or "g11_parse_pred" in only:
        make_parse_golden(ref)
    if not only or "g12_f1" in only:
        make_f1_golden(ref)
    if not only or "g13_lr_schedule" in only:
        make_lr_golden(ref)
    if not only or "g22_reference_ops" in only:
        make_reference_ops_golden(ref)


REFERENCE_OPS_SHAPES = {"cfg1": dict(V=2, h=60, w=80, Q=64, I=1), "cfg2_shape_fp32": dict(V=5, h=120, w=160, Q=128, I=4),
                        "cfg3": dict(V=10, h=120, w=160, Q=256, I=8)}
REFERENCE_OPS_SEEDS = dict(wseed=901, sseed=902)


def reference_ops_case_inputs(sh):
    cfg = synth.decoder_cfg(dim=256, queries=sh["Q"], heads=4, ffn=768, layers=sh["I"])
    W = synth.make_decoder_weights(cfg, REFERENCE_OPS_SEEDS["wseed"])
    sc = synth.make_scene(REFERENCE_OPS_SEEDS["sseed"], 1, sh["V"], sh["h"], sh["w"], 256)
    return cfg, W, sc


def make_reference_ops_golden(ref):
    arrays = {}
    for name, sh in REFERENCE_OPS_SHAPES.items():
        cfg, W, sc = reference_ops_case_inputs(sh)
        dec = RL.build_reference_decoder(ref, cfg, W)
        t = torch.from_numpy
        with torch.no_grad():
            outs = dec(t(sc["tokens"]), ref.Camera(t(sc["camera"])), ref.Pose(t(sc["T_camera_pseudoCam"])),
                       ref.Pose(t(sc["T_world_pseudoCam"])), ref.Pose(t(sc["T_world_local"])))
        for k, o in enumerate(outs):
            for key in KEYS:
                arrays["%s_it%d_%s" % (name, k, key)] = o[key].detach().numpy().astype(np.float32)
    meta = dict(shapes=REFERENCE_OPS_SHAPES, **REFERENCE_OPS_SEEDS)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT_DIR, "g22_reference_ops.npz"), **arrays)
    print("wrote g22_reference_ops", len(arrays) - 1, "arrays")


PARSE_CASE = dict(seed=41, B=2, Q=96, track_scale=[-1.5, 1.5, -2, 1, 0, 2])


def parse_case_inputs(c):
    """Last-iteration outputs for the parse_pred golden: clustered boxes so that the NMS has work to do."""
    rng = np.random.RandomState(c["seed"])
    B, Q = c["B"], c["Q"]
    anchors = rng.uniform(-1.2, 1.2, (B, 12, 3)) * np.array([1.0, 0.5, 1.0]) + np.array([0.0, -0.5, 1.0])
    which = rng.randint(0, 12, (B, Q))
    center = np.take_along_axis(anchors, which[..., None].repeat(3, -1), 1) + rng.normal(0, 0.08, (B, Q, 3))
    center[:, :6] += rng.uniform(-3, 3, (B, 6, 3))                         # some outside the validity window
    size = rng.uniform(0.3, 0.9, (B, Q, 3))
    rot6 = rng.normal(0, 1, (B, Q, 6))
    logits = rng.normal(0, 1.5, (B, Q, 10))
    prob = np.exp(logits) / np.exp(logits).sum(-1, keepdims=True)
    return {k: v.astype(np.float32) for k, v in dict(center=center, size=size, rot6=rot6, prob=prob).items()}


def make_parse_golden(ref):
    """parse_pred of the reference (model/parq_decoder.py:372-424) evaluated piecewise on the CPU: the method itself hard-codes
    .cuda(); its building blocks (ortho6d -> R, Pose.from_Rt, Obb3D.separate_init, utils/nms.nms) are the reference's own."""
    import importlib
    if not hasattr(np, "bool"):
        np.bool = bool                                   # utils/nms.py:46 predates numpy 2
    nms_mod = importlib.import_module("utils.nms")
    o6 = importlib.import_module("utils.ortho6d_transforms")
    c = PARSE_CASE
    x = {k: torch.from_numpy(v) for k, v in parse_case_inputs(c).items()}
    B, Q = c["B"], c["Q"]
    scores, labels = torch.max(x["prob"], -1)
    Rm = o6.compute_rotation_matrix_from_ortho6d(x["rot6"].contiguous().view(-1, 6)).view(B, -1, 3, 3)
    T = ref.Pose.from_Rt(Rm, x["center"])
    s = x["size"]
    c3o = torch.stack([-s[..., 0] / 2, s[..., 0] / 2, -s[..., 1] / 2, s[..., 1] / 2, -s[..., 2] / 2, s[..., 2] / 2], dim=-1)
    obbs = ref.Obb3D.separate_init(bb3_object=c3o, T_world_object=T._data, sem_id=labels)
    ts = c["track_scale"]
    cp = x["center"]
    valid = (cp[..., 0] > ts[0]) & (cp[..., 0] < ts[1]) & (cp[..., 2] > ts[4]) & (cp[..., 2] < ts[5])
    m_eval = torch.tensor(nms_mod.nms(obbs, scores, 9, 0.1, "nms_3d_faster")) & valid
    m_vis = torch.tensor(nms_mod.nms(obbs, scores, 9, 0.2, "nms_3d_faster_samecls"))
    np.savez_compressed(os.path.join(OUT_DIR, "g11_parse_pred.npz"), obbs=obbs._data.numpy(), mask_eval=m_eval.numpy(),
                        mask_vis=m_vis.numpy(), meta=np.frombuffer(json.dumps(c, sort_keys=True).encode(), dtype=np.uint8))
    print("wrote g11_parse_pred: kept", int(m_eval.sum()), "of", B * Q, "(eval),", int(m_vis.sum()), "(vis)")


LOSS_CASE = dict(seed=31, B=3, Q=48, I=2, nbox=[4, 6, 3], np_seed=1234)    # (the reference raises on a scene without boxes)


def loss_case_inputs(c):
    """Random decoder outputs, padded ground-truth boxes, poses and symmetry classes of the loss golden (numpy)."""
    B, Q, I = c["B"], c["Q"], c["I"]
    rng = np.random.RandomState(c["seed"])
    obbs = -np.ones((B, 12, 19), np.float32)
    sym = -np.ones((B, 12), np.float32)
    centers = []
    for b in range(B):
        cb = []
        for j in range(c["nbox"][b]):
            half = rng.uniform(0.2, 0.8, 3)
            ang = rng.uniform(-np.pi, np.pi)
            Rm = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
            t = rng.uniform(-1.5, 1.5, 3)
            obbs[b, j, 0:6] = [-half[0], half[0], -half[1], half[1], -half[2], half[2]]
            obbs[b, j, 6:15] = Rm.reshape(-1)
            obbs[b, j, 15:18] = t
            obbs[b, j, 18] = rng.randint(0, 9)
            sym[b, j] = rng.randint(0, 4)
            cb.append(t)
        centers.append(cb)
    T_wl = np.zeros((B, 1, 12), np.float32)
    for b in range(B):
        ang = rng.uniform(-0.3, 0.3)
        T_wl[b, 0, :9] = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]).reshape(-1)
        T_wl[b, 0, 9:] = rng.uniform(-0.2, 0.2, 3)
    outs = []
    for k in range(I):
        o = {"pred_logits": rng.normal(0, 1, (B, Q, 10)).astype(np.float32),
             "center_unnormalized": rng.uniform(-2, 2, (B, Q, 3)).astype(np.float32),
             "size_unnormalized": rng.uniform(0.2, 2, (B, Q, 3)).astype(np.float32),
             "ortho6d": rng.normal(0, 1, (B, Q, 6)).astype(np.float32),
             "coord_pos": rng.uniform(-2, 2, (B, Q, 3)).astype(np.float32)}
        # a cluster of reference points around the first boxes: exercises the proximity matching and its cap of 10
        for b in range(B):
            if centers[b]:
                # centres are in world coordinates; the matcher compares in the local frame: close enough for T_wl ~ identity
                o["coord_pos"][b, :14] = (np.asarray(centers[b][0]) + rng.uniform(-0.04, 0.04, (14, 3))).astype(np.float32)
                if len(centers[b]) > 1:
                    o["coord_pos"][b, 14:18] = (np.asarray(centers[b][1]) + rng.uniform(-0.04, 0.04, (4, 3))).astype(np.float32)
        outs.append(o)
    return outs, obbs, T_wl, sym


def make_loss_golden(ref):
    c = LOSS_CASE
    outs, obbs, T_wl, sym = loss_case_inputs(c)
    cfg = synth.decoder_cfg(dim=64, queries=c["Q"], heads=1, ffn=64, layers=c["I"])
    cfg.MEAN_SIZE_PATH = ref.mean_size_path
    dec = ref.PARQDecoder(cfg)
    touts = [{k: torch.from_numpy(v) for k, v in o.items()} for o in outs]
    res = {}
    for tag, s in (("sym", torch.from_numpy(sym)), ("nosym", None)):
        np.random.seed(c["np_seed"])
        ld = dec.loss(touts, ref.Obb3D(torch.from_numpy(obbs)), ref.Pose(torch.from_numpy(T_wl)), s)
        for k, v in ld.items():
            res["%s_%s" % (tag, k)] = np.float64(float(v))
    np.savez_compressed(os.path.join(OUT_DIR, "g10_loss.npz"), meta=np.frombuffer(json.dumps(c, sort_keys=True).encode(), dtype=np.uint8), **res)
    print("wrote g10_loss", {k: float(v) for k, v in res.items()})


F1_CASE = dict(seed=53, scenes=["scene_a", "scene_b", "scene_c"], snippets=4, Q=40, ngt=7, np_seed=4321, conf=0.1)


def _yaw_box_corners(center, half, yaw):
    """World corners (8,3) of a box rotated about the world z axis, in the corner order of Obb3D.bb3corners_object with the
    object's y axis along world +z (the convention the reference's IoU routine assumes, utils/f1_eval.py:77-100)."""
    sx, sy, sz = half
    obj = np.array([[-sx, -sy, -sz], [sx, -sy, -sz], [sx, sy, -sz], [-sx, sy, -sz],
                    [-sx, -sy, sz], [sx, -sy, sz], [sx, sy, sz], [-sx, sy, sz]])
    c, s_ = np.cos(yaw), np.sin(yaw)
    Rz = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]])
    R0 = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])          # object y -> world +z
    return obj @ (Rz @ R0).T + center


def f1_case_inputs(c):
    """Per snippet: predicted corners / class probabilities / mask for every scene, and the visible ground truth.
    Predictions are noisy copies of the scene's boxes plus clutter, so tracks merge, get replaced and new ones appear."""
    rng = np.random.RandomState(c["seed"])
    S, Q = len(c["scenes"]), c["Q"]
    world = []
    for s_ in range(S):
        boxes = []
        for j in range(c["ngt"]):
            boxes.append(dict(center=rng.uniform(-2.5, 2.5, 3) * np.array([1, 1, 0.3]), half=rng.uniform(0.25, 0.7, 3),
                              yaw=rng.uniform(-np.pi, np.pi), cls=int(rng.randint(0, 9))))
        world.append(boxes)
    steps = []
    for t in range(c["snippets"]):
        order = list(range(S)) if t % 2 == 0 else [2, 0]                 # a ragged batch and a different scene order
        corners = np.zeros((len(order), Q, 8, 3), np.float32)
        prob = np.zeros((len(order), Q, 10), np.float32)
        mask = np.zeros((len(order), Q), bool)
        gts = []
        for bi, s_ in enumerate(order):
            vis = [j for j in range(c["ngt"]) if rng.rand() < 0.7]
            gts.append(dict(labels=np.array([world[s_][j]["cls"] for j in vis], np.int64),
                            corners=np.stack([_yaw_box_corners(world[s_][j]["center"], world[s_][j]["half"], world[s_][j]["yaw"])
                                              for j in vis]).astype(np.float32) if vis else np.zeros((0, 8, 3), np.float32)))
            for q in range(Q):
                logits = rng.normal(0, 1, 10)
                if q < 2 * c["ngt"] and rng.rand() < 0.75:                 # a detection of box q % ngt
                    bx = world[s_][q % c["ngt"]]
                    cen = bx["center"] + rng.normal(0, 0.10, 3)
                    half = bx["half"] * rng.uniform(0.75, 1.25, 3)
                    yaw = bx["yaw"] + rng.normal(0, 0.15)
                    logits[bx["cls"] if rng.rand() < 0.85 else rng.randint(0, 10)] += rng.uniform(1.5, 4.0)
                else:                                                      # clutter
                    cen = rng.uniform(-3, 3, 3) * np.array([1, 1, 0.3])
                    half = rng.uniform(0.2, 0.6, 3)
                    yaw = rng.uniform(-np.pi, np.pi)
                    logits[9] += rng.uniform(0.0, 3.0)
                corners[bi, q] = _yaw_box_corners(cen, half, yaw)
                e = np.exp(logits - logits.max())
                prob[bi, q] = e / e.sum()
                mask[bi, q] = rng.rand() < 0.8
        steps.append(dict(scenes=[c["scenes"][s_] for s_ in order], corners=corners, prob=prob, mask=mask, gts=gts))
    return steps


def make_f1_golden(ref):
    """The reference's F1Calculator (utils/f1_eval.py:254-557) driven snippet by snippet through step(); the jitter it adds to
    the ground truth draws from NumPy's global generator, seeded here."""
    import importlib
    f1 = importlib.import_module("utils.f1_eval")
    c = F1_CASE
    steps = f1_case_inputs(c)
    calc = f1.F1Calculator(c["conf"])
    np.random.seed(c["np_seed"])
    import contextlib, io
    for st in steps:
        out = {"pred_corners_world": torch.from_numpy(st["corners"]), "sem_cls_prob": torch.from_numpy(st["prob"]),
               "pred_mask": torch.from_numpy(st["mask"]), "scene_name": st["scenes"]}
        gl = [{"labels": torch.from_numpy(g["labels"]), "gt_corners_world": torch.from_numpy(g["corners"])} for g in st["gts"]]
        calc.step(out, gl)
    with contextlib.redirect_stdout(io.StringIO()):
        metrics = calc.compute_metrics()
    res = {"metric_" + k: np.float64(v) for k, v in metrics.items()}
    for name in c["scenes"]:
        res["ntrack_" + name] = np.int64(len(calc.preds[name]))
        res["ngt_" + name] = np.int64(len(calc.gts[name]))
        res["trackcls_" + name] = np.array([t[0] for t in calc.preds[name]], np.int64)
        res["trackid_" + name] = np.array([t[-1] for t in calc.preds[name]], np.int64)
        res["trackscore_" + name] = np.array([t[2] for t in calc.preds[name]], np.float64)
    # a few raw IoUs of the reference routine, for the IoU restatement on its own
    rng = np.random.RandomState(7)
    pairs, ious = [], []
    rot = f1.rotx(np.pi / 2)
    for _ in range(24):
        cen = rng.uniform(-1, 1, 3) * np.array([1, 1, 0.2])
        a = _yaw_box_corners(cen, rng.uniform(0.3, 0.8, 3), rng.uniform(-np.pi, np.pi))
        b = _yaw_box_corners(cen + rng.normal(0, 0.35, 3) * np.array([1, 1, 0.3]), rng.uniform(0.3, 0.8, 3), rng.uniform(-np.pi, np.pi))
        ra = (rot @ a[[4, 0, 1, 5, 7, 3, 2, 6]].T).T
        rb = (rot @ b[[4, 0, 1, 5, 7, 3, 2, 6]].T).T
        with contextlib.redirect_stdout(io.StringIO()):
            i3, i2 = f1.iou3d(ra, rb)
        pairs.append(np.stack([a, b]))
        ious.append([i3, i2])
    res["iou_pairs"] = np.stack(pairs)
    res["iou_values"] = np.array(ious, np.float64)
    np.savez_compressed(os.path.join(OUT_DIR, "g12_f1.npz"), meta=np.frombuffer(json.dumps(c, sort_keys=True).encode(), dtype=np.uint8), **res)
    print("wrote g12_f1", {k: float(v) for k, v in metrics.items()}, [int(res["ntrack_" + n]) for n in c["scenes"]])


LR_CASES = [dict(first=10, mult=1.0, max_lr=1e-3, min_lr=1e-5, warmup=3, steps=35),
            dict(first=7, mult=2.0, max_lr=4e-4, min_lr=4e-4 / 256, warmup=0, steps=40),
            dict(first=12, mult=1.5, max_lr=2e-3, min_lr=1e-6, warmup=5, steps=60)]


def make_lr_golden(ref):
    """Learning-rate sequences of the reference's CosineAnnealingWarmupRestarts (utils/train_utils.py:18-145), stepped once
    per epoch as Lightning does (model/parq_lightning.py:183-199)."""
    import importlib
    tu = importlib.import_module("utils.train_utils")
    res = {}
    for i, c in enumerate(LR_CASES):
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=c["max_lr"])
        sch = tu.CosineAnnealingWarmupRestarts(opt, c["first"], c["mult"], c["max_lr"], c["min_lr"], c["warmup"])
        seq = [opt.param_groups[0]["lr"]]
        for _ in range(c["steps"]):
            opt.step()
            sch.step()
            seq.append(opt.param_groups[0]["lr"])
        res["lr_%d" % i] = np.array(seq, np.float64)
    np.savez_compressed(os.path.join(OUT_DIR, "g13_lr_schedule.npz"),
                        meta=np.frombuffer(json.dumps(LR_CASES, sort_keys=True).encode(), dtype=np.uint8), **res)
    print("wrote g13_lr_schedule", [len(v) for v in res.values()])


def scan_self_noise(base, pairs):
    """`python -m oracle.make_golden scan <case> w:s [w:s ...]`: the reference's own fp32-vs-float64 deviation (largest
    |a-b| / max(1,|b|) over decision-safe elements, float64 oracle teacher-forced on the reference's reference points) of case
    `base` under other (weight seed, scene seed) pairs — how the seeds of the unrelaxed fixtures are chosen."""
    ref = RL.load()
    for ws, ss in pairs:
        case = dict(CASES[base], wseed=ws, sseed=ss)
        cfg, W, sc, outs = run_reference(ref, case)
        mg = margins(cfg, W, sc, outs)
        od = O.OracleDecoder(cfg, W, synth.SCANNET_MEAN_SIZES, dtype=torch.float64)
        od.prepare(sc["tokens"], sc["camera"], sc["T_camera_pseudoCam"], sc["T_world_pseudoCam"], sc["T_world_local"])
        worst = 0.0
        for k, o in enumerate(outs):
            ref_k = O.normalize(o["coord_pos"].double(), cfg.TRANSFORMER.SCALE)
            exact = od.iterate(ref_k, k)[0]
            vm = torch.from_numpy(mg["it%d_valid_margin" % k] > 2e-3)
            cm = torch.from_numpy(mg["it%d_cls_margin" % k] > 1e-3)
            for key in KEYS:
                if key == "coord_pos":
                    continue
                m = vm & cm if key == "size_unnormalized" else vm
                e = ((o[key].double() - exact[key]).abs() / exact[key].abs().clamp(min=1))[m]
                worst = max(worst, float(e.max()) if e.numel() else 0.0)
        print("%s wseed %d sseed %d: reference fp32 vs float64 %.2e" % (base, ws, ss, worst), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "scan":
        scan_self_noise(sys.argv[2], [tuple(int(x) for x in a.split(":")) for a in sys.argv[3:]])
        sys.exit(0)
    main(sys.argv[1:] or None)
