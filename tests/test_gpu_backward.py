"""Backward of the decoder chain against autograd of the float64 oracle.

The oracle (oracle/parq_oracle.py) is plain torch, so `loss = sum_k <cotangent_k, output_k>` differentiated by autograd in
float64 gives the reference gradients for every weight and for the input tokens.  As in the reference, the reference points
are detached between iterations (model/transformer_parq.py:331-332); iteration 0 differentiates through
sigmoid(refpoint.weight).  Tolerance per tensor: Frobenius-relative error < 2e-3 and max-norm-relative error < 2e-2 (fp32 chain
with atomics against float64; a ReLU whose pre-activation sits within rounding of zero flips its mask between the two
precisions and moves single gradient entries, which the max-norm bound allows for and the Frobenius bound averages).
"""
import numpy as np
import pytest
import torch

from parq_amd import synth
from oracle import parq_oracle as O
from gpu_util import make_decoder, scene_args

pytestmark = pytest.mark.gpu

GKEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d")


def oracle_grads(cfg, W, sc, cots):
    od = O.OracleDecoder(cfg, W, synth.SCANNET_MEAN_SIZES, dtype=torch.float64)
    for k in od.W:
        od.W[k].requires_grad_(True)
    od.prepare(sc["tokens"], sc["camera"], sc["T_camera_pseudoCam"], sc["T_world_pseudoCam"], sc["T_world_local"])
    od.tokens.requires_grad_(True)
    ref = od.initial_ref()
    loss = 0.0
    outs = []
    for k in range(cfg.TRANSFORMER.DEC_LAYERS):
        out, nxt, _ = od.iterate(ref, k)
        outs.append(out)
        for key in GKEYS:
            loss = loss + (out[key] * torch.from_numpy(cots[key][k]).double()).sum()
        ref = nxt.detach()
    loss.backward()
    grads = {k: v.grad for k, v in od.W.items() if v.grad is not None}
    return grads, od.tokens.grad, outs


@pytest.mark.parametrize("B,V,h,w,Q,heads,dim,ffn,layers,shared", [
    (2, 2, 8, 10, 32, 2, 128, 96, 2, True),
    (1, 3, 6, 7, 40, 4, 256, 256, 3, True),
    (2, 2, 5, 6, 16, 2, 128, 64, 2, False),
    (2, 2, 32, 40, 40, 2, 128, 96, 2, True),       # N = 2560 keys: the MFMA cross-attention backward with dQ partial buffers
    (2, 2, 32, 41, 24, 4, 256, 128, 3, True),      # d = 256, N = 2624 (ragged 32-row steps): batched backward + split-precision dW_kv
    (2, 2, 9, 11, 40, 1, 256, 96, 2, True),        # head dim 256 (the reference's shipped head size): all iterations in one composition
                                                   # of split-precision GEMMs (S^T, dP^T, dV, dK; dQ by the 512 x 256 TN kernel)
    (1, 2, 32, 41, 24, 4, 1024, 256, 3, True),     # the shipped dims themselves (d = 1024, 4 heads of 256), N = 2624, three iterations
                                                   # (dW of the C = 1024 layers: the 64 x 64 tiled TN kernel, 24 rows = one partial row step)
    (2, 1, 12, 16, 40, 4, 1024, 3072, 2, True),    # the same with the shipped FFN width (3072) and 80 rows (two row steps + 16)
    (1, 2, 10, 13, 20, 2, 256, 96, 2, False),      # head dim 128, unshared layers, ragged key count (N = 260)
])
def test_backward_matches_oracle_autograd(B, V, h, w, Q, heads, dim, ffn, layers, shared):
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=heads, ffn=ffn, layers=layers, share_weights=shared, dropout=0.0)
    # damped centre head: the comparison is FREE-RUNNING over 2-3 iterations, and with the undamped head a
    # rounding-level difference of the forward (1e-6: e.g. another summation order in the split merge) grows to 1e-2 in the centre
    # head's gradients by the third iteration — a property of the fixture (measured: two fp32 summation orders of the same kernels
    # differ by that much from each other), not of the backward
    W = synth.make_decoder_weights(cfg, 71, damped=True)
    sc = synth.make_scene(72, B, V, h, w, dim, smooth=True)
    ncls = cfg.NUM_SEMCLS + 1
    cots = {"pred_logits": synth.normal(73, "cl", (layers, B, Q, ncls)), "center_unnormalized": synth.normal(74, "cc", (layers, B, Q, 3)),
            "size_unnormalized": synth.normal(75, "cs", (layers, B, Q, 3)), "ortho6d": synth.normal(76, "cr", (layers, B, Q, 6))}
    want, want_tok, oouts = oracle_grads(cfg, W, sc, cots)

    dec = make_decoder(cfg, W)
    dec.attention_mode = "fp32"
    outs = dec.forward_train(*scene_args(sc))
    for k in range(layers):                                   # the training forward is the same forward
        for key in GKEYS:
            a, b = outs[k][key].cpu().numpy(), oouts[k][key].detach().numpy()
            assert np.abs(a - b).max() / max(1.0, np.abs(b).max()) < 1e-4, (k, key)
    grads, d_tok = dec.backward({k: torch.from_numpy(v) for k, v in cots.items()})
    worst = {}
    for name, g in grads.items():
        if name not in want:
            assert float(g.abs().max()) == 0.0, name          # e.g. never-used tensors
            continue
        ref = want[name].numpy()
        d = g.cpu().numpy().astype(np.float64) - ref
        worst[name] = (np.linalg.norm(d) / max(np.linalg.norm(ref), 1e-9), np.abs(d).max() / max(np.abs(ref).max(), 1e-9))
    bad = {k: v for k, v in worst.items() if not (v[0] < 2e-3 and v[1] < 2e-2)}
    print("\nworst relative gradient errors (frobenius, max):", sorted(worst.items(), key=lambda kv: -kv[1][0])[:5])
    assert not bad, bad
    rt = want_tok.numpy()
    dt = d_tok.cpu().numpy().astype(np.float64) - rt
    terr = (np.linalg.norm(dt) / max(np.linalg.norm(rt), 1e-9), np.abs(dt).max() / max(np.abs(rt).max(), 1e-9))
    print("token gradient error (frobenius, max) %.3e %.3e" % terr)
    assert terr[0] < 2e-3 and terr[1] < 2e-2, terr


def test_autograd_node_and_adamw_steps():
    """PARQDecoder in train mode under autograd: loss.backward() fills .grad of every parameter and of the input tokens
    through the HIP backward, and a few AdamW steps (model/parq_lightning.py:161-199: AdamW, lr 1e-4 scale) lower a
    regression loss on fixed targets."""
    B, V, h, w, Q, dim = 2, 2, 8, 10, 32, 128
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=2, ffn=96, layers=2, dropout=0.0)
    W = synth.make_decoder_weights(cfg, 81)
    sc = synth.make_scene(82, B, V, h, w, dim, smooth=True)
    dec = make_decoder(cfg, W).train()
    args = list(scene_args(sc))
    args[0] = args[0].clone().requires_grad_(True)
    cots = {k: torch.from_numpy(synth.normal(83 + i, k, (2, B, Q, wd))).cuda()
            for i, (k, wd) in enumerate((("pred_logits", cfg.NUM_SEMCLS + 1), ("center_unnormalized", 3), ("size_unnormalized", 3), ("ortho6d", 6)))}
    outs = dec(*args)
    loss = sum((outs[k][key] * cots[key][k]).sum() for k in range(2) for key in GKEYS)
    loss.backward()
    np_cots = {k: v.cpu().numpy() for k, v in cots.items()}
    want, want_tok, _ = oracle_grads(cfg, W, sc, np_cots)
    seen = 0
    for name, p in dec.named_parameters():
        if name in want and p.grad is not None:
            ref = want[name].numpy()
            assert np.linalg.norm(p.grad.cpu().numpy() - ref) / max(np.linalg.norm(ref), 1e-9) < 2e-3, name
            seen += 1
    assert seen >= 30
    rt = want_tok.numpy()
    assert np.linalg.norm(args[0].grad.cpu().numpy() - rt) / np.linalg.norm(rt) < 2e-3

    opt = torch.optim.AdamW([p for p in dec.parameters() if p.requires_grad], lr=2e-3, weight_decay=1e-4)
    target = torch.from_numpy(synth.uniform(90, "tgt", (B, Q, 3), -1.0, 1.0)).cuda()
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        outs = dec(*scene_args(sc))
        l = sum(((o["center_unnormalized"] - target) ** 2).mean() for o in outs)
        l.backward()
        torch.nn.utils.clip_grad_norm_(dec.parameters(), 1.0)            # parq_lightning.py gradient_clip_val = 1
        opt.step()
        losses.append(float(l))
    print("\nregression loss over AdamW steps:", ["%.4f" % x for x in losses])
    assert losses[-1] < losses[0]


def test_ray_pe_backward_matches_oracle_autograd(monkeypatch):
    """AddRayPE.tokens as an autograd node: gradients of encoder.{0,2}.{weight,bias} and of the feature maps against float64
    autograd of the oracle's ray_pe + tokenize (tiles straddle views; d = 256 is the fused forward path)."""
    from parq_amd import AddRayPE
    B, V, h, w, Cd = 2, 3, 7, 9, 256
    scale = [-3.0, 3.0, -2.0, 0.5, 0.25, 5.25]
    Wp = synth.make_ray_pe_weights(Cd, 91)
    cam, T_cp, T_wp, T_wl = synth.make_geometry(92, B, V, h, w)
    feat = synth.normal(93, "feat", (B, V, Cd, h, w))
    cot = synth.normal(94, "cot", (B, V * h * w, Cd))
    # oracle, float64, leaf tensors passed through unchanged
    W64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in Wp.items()}
    f64 = torch.from_numpy(feat).double().requires_grad_(True)
    monkeypatch.setattr(O, "_as_torch", lambda Wd, dtype: Wd)
    enc = O.ray_pe(cam, T_cp, T_wp, T_wl, W64, scale, dtype=torch.float64)
    (O.tokenize(f64, enc) * torch.from_numpy(cot).double()).sum().backward()

    pe = AddRayPE(Cd, scale, 64, 0.25, 5.25)
    pe.load_state_dict({k: torch.from_numpy(v) for k, v in Wp.items()}, strict=True)
    pe = pe.cuda().train()
    fg = torch.from_numpy(feat).cuda().requires_grad_(True)
    tok = pe.tokens(fg, *(torch.from_numpy(x).cuda() for x in (cam, T_cp, T_wp, T_wl)))
    (tok * torch.from_numpy(cot).cuda()).sum().backward()
    for name, p in pe.named_parameters():
        ref = W64[name].grad.numpy()
        err = np.linalg.norm(p.grad.cpu().numpy() - ref) / np.linalg.norm(ref)
        assert err < 1e-4, (name, err)
    ref = f64.grad.numpy()
    assert np.abs(fg.grad.cpu().numpy() - ref).max() < 1e-6


@pytest.mark.parametrize("Cd,heads,ffn,layers,pdrop,lr", [(128, 2, 96, 2, 0.0, 2e-3),
                                                           (1024, 4, 3072, 3, 0.1, 1e-4)])    # the reference's shipped recipe: DEC_DIM 1024, 4 heads
                                                                                              # of 256, FFN 3072, dropout 0.1 (config/train.yaml:45-56)
def test_parq_module_training_steps_with_set_loss(Cd, heads, ffn, layers, pdrop, lr):
    """PARQ.training_step end to end (model/parq_lightning.py:97-100): ray-PE node -> decoder node -> the reference's set loss
    on synthetic boxes; every parameter of the encoder MLP and of the decoder receives a gradient and AdamW lowers the loss."""
    from types import SimpleNamespace as NS
    from parq_amd import PARQ, Camera, Obb3D, Pose
    B, V, h, w, Qn = 2, 2, 8, 10, 32
    dcfg = synth.decoder_cfg(dim=Cd, queries=Qn, heads=heads, ffn=ffn, layers=layers, dropout=pdrop)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg), OPTIMIZER=NS(LEARNING_RATE=lr, AUTOSCALE_LR=False))
    torch.manual_seed(0)
    model = PARQ(cfg).cuda().train()
    cam, T_cp, T_wp, T_wl = synth.make_geometry(95, B, V, h, w)
    obbs, sym = synth.make_boxes(96, B, 5, max_box=8)
    to = lambda a: torch.from_numpy(a).cuda()
    batch = {"all_features": to(synth.normal(97, "f", (B, V, Cd, h, w), std=0.5)), "camera_feature": Camera(to(cam)),
             "T_camera_pseudoCam": Pose(to(T_cp)), "T_world_pseudoCam": Pose(to(T_wp)), "T_world_local": Pose(to(T_wl)),
             "obbs_padded": Obb3D(to(obbs)), "sym": to(sym)}
    opt = model.configure_optimizers()
    np.random.seed(5)
    losses = []
    for it in range(5):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, it)
        loss.backward()
        if it == 0:
            missing = [n for n, p in model.named_parameters() if p.grad is None and "decoder.norm." not in n]
            assert not missing, missing
            assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
            assert float(model.add_ray_pe.encoder[0].weight.grad.abs().max()) > 0
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        losses.append(float(loss.detach()))
    print("\nset loss over AdamW steps:", ["%.4f" % x for x in losses])
    assert losses[-1] < losses[0]


def _masked_mha(xq, xk, xv, in_w, in_b, out_w, out_b, H, pmask):
    """nn.MultiheadAttention forward with an explicit keep-mask (already scaled by 1/(1-p)) on the probabilities."""
    Cd = xq.shape[-1]
    dh = Cd // H
    q = torch.nn.functional.linear(xq, in_w[:Cd], in_b[:Cd])
    k = torch.nn.functional.linear(xk, in_w[Cd:2 * Cd], in_b[Cd:2 * Cd])
    v = torch.nn.functional.linear(xv, in_w[2 * Cd:], in_b[2 * Cd:])
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    q = q.view(B, Lq, H, dh).transpose(1, 2); k = k.view(B, Lk, H, dh).transpose(1, 2); v = v.view(B, Lk, H, dh).transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) / dh ** 0.5, -1) * pmask.view(B, H, Lq, Lk)
    return torch.nn.functional.linear((p @ v).transpose(1, 2).reshape(B, Lq, Cd), out_w, out_b)


@pytest.mark.parametrize("h,w,Hh,dim,mode", [(8, 10, 2, 128, None), (32, 40, 2, 128, None), (8, 10, 1, 128, None), (12, 14, 1, 256, None),
                                             (32, 36, 4, 256, None), (32, 38, 4, 256, None),   # these two: mode "split8" in training (opt-in; N = 2304 / 2432 = whole 64-key stages, the second not whole 256-key backward tiles)
                                             (32, 36, 4, 256, "fp16"), (32, 38, 4, 256, "bf16"),   # the single-product dropout kernels on whole stages (flash_split8_kernel<..., DROP, 1, kind>)
                                             (8, 10, 8, 256, None), (32, 40, 8, 256, None)])   # head dim 32: attn_bwd_kernel<32>, launch_self_attn
                                                                              # N = 160: exact-fp32 attention backward; N = 2560: split-precision
                                                                              # kernel; one head of 128 dims: materialised backward;
                                                                              # one head of 256 dims: the batched composition from split GEMMs
def test_dropout_forward_backward_match_masked_oracle(h, w, Hh, dim, mode):
    """Train-mode dropout (six sites of the decoder layer, transformer_parq.py:339-386): the library's counter-based masks are
    dumped (parq_k_dropout_mask) and applied at the same sites in a float64 torch restatement of the layer; outputs and all
    gradients must then agree like in the dropout-free test.  Also: masks change with the seed, the drop rate is ~p."""
    import ctypes as C
    from parq_amd import _lib
    F_ = torch.nn.functional
    B, V, Q, ffn, I = 2, 2, 32, 96, 2
    pdrop = 0.25
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=Hh, ffn=ffn, layers=I, dropout=pdrop)
    W = synth.make_decoder_weights(cfg, 101)
    sc = synth.make_scene(102, B, V, h, w, dim, smooth=True)
    ncls = cfg.NUM_SEMCLS + 1
    cots = {"pred_logits": synth.normal(103, "cl", (I, B, Q, ncls)), "center_unnormalized": synth.normal(104, "cc", (I, B, Q, 3)),
            "size_unnormalized": synth.normal(105, "cs", (I, B, Q, 3)), "ortho6d": synth.normal(106, "cr", (I, B, Q, 6))}
    dec = make_decoder(cfg, W).train()
    dec.train_split8 = True                   # takes effect where mode 4 applies (d = 256, head dim 64, whole stages, batched backward)
    if mode:
        dec.attention_mode = mode
    assert (dec._train_mode() == "split8") == ((dim, Hh) == (256, 4) and not mode)
    # 16-bit modes: the gradient bounds of test_training_in_reduced_precision_attention_modes (measured here 8e-3 / 2.2e-2), its output
    # bounds times 3 (this fixture is free-running on UNDAMPED weights with the kept probabilities scaled by 1 / 0.75; measured 5.4e-4 /
    # 2.1e-3); a mask that differed between forward and backward would show as O(1)
    out_tol, grad_tol = {None: (1e-4, 2e-3), "fp16": (1e-3, 2e-2), "bf16": (6e-3, 5e-2)}[mode]
    torch.manual_seed(7)
    outs = dec.forward_train(*scene_args(sc))
    N, M = V * h * w, B * Q
    lib, hd = _lib.load(), dec._handle(apply_mode=False)

    def mask(k, site, rows, cols):
        t = torch.empty(rows, cols, device="cuda")
        _lib.check(lib.parq_k_dropout_mask(hd, k, site, rows, cols, _lib.ptr(t), _lib.stream_ptr()), "mask")
        return t.cpu().double()
    shapes = {0: (B * Hh * Q, Q), 1: (M, dim), 2: (B * Hh * Q, N), 3: (M, dim), 4: (M, ffn), 5: (M, dim)}
    masks = {(k, s): mask(k, s, *shapes[s]) for k in range(I) for s in range(6)}
    frac = float((masks[(0, 2)] == 0).double().mean())
    assert abs(frac - pdrop) < 0.01, frac
    assert not torch.equal(masks[(0, 1)], masks[(1, 1)])

    # float64 restatement with the same masks
    od = O.OracleDecoder(cfg, W, synth.SCANNET_MEAN_SIZES, dtype=torch.float64)
    for kk in od.W:
        od.W[kk].requires_grad_(True)
    od.prepare(sc["tokens"], sc["camera"], sc["T_camera_pseudoCam"], sc["T_world_pseudoCam"], sc["T_world_local"])
    od.tokens.requires_grad_(True)
    Wd = od.W
    ref = od.initial_ref()
    loss = 0.0
    oouts = []
    d = "parq_module.decoder.position_encoder."
    p = "parq_module.decoder.layers.0."
    for k in range(I):
        pos = F_.linear(F_.relu(F_.linear(O.pos2posemb3d(ref), Wd[d + "0.weight"], Wd[d + "0.bias"])), Wd[d + "2.weight"], Wd[d + "2.bias"])
        tgt, _, _ = O.project_and_sample(od.tokens, O.denormalize(ref, cfg.TRANSFORMER.SCALE), od.T_cl, od.cam, od.h, od.w)
        qk = tgt + pos
        sa = _masked_mha(qk, qk, tgt, Wd[p + "self_attn.in_proj_weight"], Wd[p + "self_attn.in_proj_bias"],
                         Wd[p + "self_attn.out_proj.weight"], Wd[p + "self_attn.out_proj.bias"], Hh, masks[(k, 0)])
        x = O.layer_norm(tgt + sa * masks[(k, 1)].view(B, Q, dim), Wd[p + "norm1.weight"], Wd[p + "norm1.bias"])
        ca = _masked_mha(x + pos, od.tokens, od.tokens, Wd[p + "multihead_attn.in_proj_weight"], Wd[p + "multihead_attn.in_proj_bias"],
                         Wd[p + "multihead_attn.out_proj.weight"], Wd[p + "multihead_attn.out_proj.bias"], Hh, masks[(k, 2)])
        x = O.layer_norm(x + ca * masks[(k, 3)].view(B, Q, dim), Wd[p + "norm2.weight"], Wd[p + "norm2.bias"])
        hid = F_.relu(F_.linear(x, Wd[p + "linear1.weight"], Wd[p + "linear1.bias"])) * masks[(k, 4)].view(B, Q, ffn)
        ff = F_.linear(hid, Wd[p + "linear2.weight"], Wd[p + "linear2.bias"])
        x = O.layer_norm(x + ff * masks[(k, 5)].view(B, Q, dim), Wd[p + "norm3.weight"], Wd[p + "norm3.bias"])
        out = O.box_heads(x, ref, Wd, cfg.TRANSFORMER.SCALE, od.mean_sizes)
        oouts.append(out)
        for key in GKEYS:
            loss = loss + (out[key] * torch.from_numpy(cots[key][k]).double()).sum()
        ref = O.normalize(out["center_unnormalized"], cfg.TRANSFORMER.SCALE).detach()
    loss.backward()
    for k in range(I):
        for key in GKEYS:
            a, b = outs[k][key].cpu().numpy(), oouts[k][key].detach().numpy()
            assert np.abs(a - b).max() / max(1.0, np.abs(b).max()) < out_tol, (k, key)
    grads, d_tok = dec.backward({k: torch.from_numpy(v) for k, v in cots.items()})
    worst = {}
    for name, g in grads.items():
        if name in Wd and Wd[name].grad is not None:
            refg = Wd[name].grad.numpy()
            dd = g.cpu().numpy().astype(np.float64) - refg
            worst[name] = np.linalg.norm(dd) / max(np.linalg.norm(refg), 1e-9)
    print("\nworst gradient errors with dropout:", sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    assert max(worst.values()) < grad_tol, max(worst.values())
    rt = od.tokens.grad.numpy()
    assert np.linalg.norm(d_tok.cpu().numpy() - rt) / np.linalg.norm(rt) < grad_tol
    # a second call draws a new seed -> different outputs; eval mode ignores dropout
    outs2 = dec.forward_train(*scene_args(sc))
    assert not torch.equal(outs2[0]["ortho6d"], outs[0]["ortho6d"])


@pytest.mark.parametrize("pdrop", [0.0, 0.2])
def test_batched_cross_attention_backward_equals_per_iteration_launches(monkeypatch, pdrop):
    """Training backward with shared layer weights: the cross-attention backward of all iterations as ONE launch (dK / dV
    accumulated in registers, written once) against the per-iteration launches that read-modify-write dK / dV
    (``backward_batched = False``: parq_set_backward_batched).  Same stash, same dropout streams; only summation order and the power-of-two dO scale differ."""
    B, V, h, w, Q, heads, dim, ffn, I = 2, 3, 32, 40, 40, 2, 128, 96, 4
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=heads, ffn=ffn, layers=I, dropout=pdrop)
    W = synth.make_decoder_weights(cfg, 171)
    sc = synth.make_scene(172, B, V, h, w, dim, smooth=True)
    ncls = cfg.NUM_SEMCLS + 1
    cots = {"pred_logits": synth.normal(173, "cl", (I, B, Q, ncls)), "center_unnormalized": synth.normal(174, "cc", (I, B, Q, 3)),
            "size_unnormalized": synth.normal(175, "cs", (I, B, Q, 3)), "ortho6d": synth.normal(176, "cr", (I, B, Q, 6))}
    res = {}
    for mode in ("1", "0"):
        dec = make_decoder(cfg, W).train()
        dec.backward_batched = mode == "1"
        torch.manual_seed(99)                                     # the dropout seed of forward_train comes from torch's generator
        dec.forward_train(*scene_args(sc))
        grads, d_tok = dec.backward({k: torch.from_numpy(v) for k, v in cots.items()})
        res[mode] = ({k: v.cpu().numpy().astype(np.float64) for k, v in grads.items()}, d_tok.cpu().numpy().astype(np.float64))
    worst = 0.0
    for name, a in res["1"][0].items():
        b = res["0"][0][name]
        if np.abs(b).max() == 0:
            assert np.abs(a).max() == 0, name
            continue
        worst = max(worst, np.linalg.norm(a - b) / np.linalg.norm(b))
    ta, tb = res["1"][1], res["0"][1]
    worst_tok = np.linalg.norm(ta - tb) / np.linalg.norm(tb)
    print("\nbatched vs per-iteration backward: worst relative difference %.2e (weights), %.2e (d tokens)" % (worst, worst_tok))
    # the batched kernel takes the probabilities and dS of its three gradient products as one fp16 value each (attn_bwd.hip, kGrad1):
    # unbiased 2^-12 noise that the contraction averages (measured 2.4e-5 here, 1.7e-5 at BASELINE cfg 3's size)
    assert worst < 5e-5 and worst_tok < 5e-5, (worst, worst_tok)


def test_backward_at_baseline_cfg3_size_batched_equals_per_iteration(monkeypatch):
    """BASELINE cfg 3 shapes (10 views 120x160 -> N = 192 000 keys, 256 queries, 8 iterations, d = 256, dropout 0.1), one scene:
    the one-launch cross-attention backward + split-precision dW_kv against the per-iteration launches + fp32 generic GEMM; all
    gradients finite, Frobenius-relative agreement 1e-4 (the oracle's autograd is out of reach at this size)."""
    V, h, w, Q, dim, I = 10, 120, 160, 256, 256, 8
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=4, ffn=768, layers=I, dropout=0.1)
    W = synth.make_decoder_weights(cfg, 41, damped=True)
    sc = synth.make_scene(272, 1, V, h, w, dim, smooth=False)
    ncls = cfg.NUM_SEMCLS + 1
    cots = {"pred_logits": synth.normal(273, "cl", (I, 1, Q, ncls)), "center_unnormalized": synth.normal(274, "cc", (I, 1, Q, 3)),
            "size_unnormalized": synth.normal(275, "cs", (I, 1, Q, 3)), "ortho6d": synth.normal(276, "cr", (I, 1, Q, 6))}
    res = {}
    for mode in ("1", "0"):
        dec = make_decoder(cfg, W).train()
        dec.backward_batched = mode == "1"
        torch.manual_seed(7)
        dec.forward_train(*scene_args(sc), feat_hw=(h, w))
        grads, d_tok = dec.backward({k: torch.from_numpy(v) for k, v in cots.items()})
        res[mode] = {k: v.double() for k, v in grads.items()}
        res[mode]["__tokens__"] = d_tok.double()
        del dec
        torch.cuda.empty_cache()
    worst = ("", 0.0)
    for name, a in res["1"].items():
        b = res["0"][name]
        assert torch.isfinite(a).all(), name
        nb = float(b.norm())
        if nb == 0:
            assert float(a.norm()) == 0, name
            continue
        rel = float((a - b).norm()) / nb
        worst = max(worst, (name, rel), key=lambda t: t[1])
        assert rel < 1e-4, (name, rel)
    print("\ncfg-3 size, batched vs per-iteration backward: worst relative difference %.2e (%s)" % (worst[1], worst[0]))


def test_head_dim_256_training_split_forward_matches_fp32_path():
    """Head dim 256 (the reference's shipped head size): the training forward on the split-precision kernels (virtual-head K/V cache,
    fp32 K / V rebuilt from it for the materialised backward) against the exact-fp32 kernels: outputs 1e-4, gradients 1e-4 relative."""
    B, V, h, w, Q, heads, dim, ffn, I = 1, 2, 24, 30, 48, 1, 256, 96, 2
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=heads, ffn=ffn, layers=I, dropout=0.0)
    W = synth.make_decoder_weights(cfg, 371)
    sc = synth.make_scene(372, B, V, h, w, dim, smooth=True)
    ncls = cfg.NUM_SEMCLS + 1
    cots = {"pred_logits": synth.normal(373, "cl", (I, B, Q, ncls)), "center_unnormalized": synth.normal(374, "cc", (I, B, Q, 3)),
            "size_unnormalized": synth.normal(375, "cs", (I, B, Q, 3)), "ortho6d": synth.normal(376, "cr", (I, B, Q, 6))}
    res = {}
    for mode in ("split", "fp32"):
        dec = make_decoder(cfg, W).train()
        dec.attention_mode = mode
        assert dec._train_mode() == mode
        outs = dec.forward_train(*scene_args(sc))
        grads, d_tok = dec.backward({k: torch.from_numpy(v) for k, v in cots.items()})
        res[mode] = ([{k: o[k].cpu().numpy() for k in GKEYS} for o in outs], {k: v.double() for k, v in grads.items()}, d_tok.double())
    for k in range(I):
        for key in GKEYS:
            a, b = res["split"][0][k][key], res["fp32"][0][k][key]
            assert np.abs(a - b).max() / max(1.0, np.abs(b).max()) < 1e-4, (k, key)
    for name, a in res["split"][1].items():
        b = res["fp32"][1][name]
        if float(b.norm()) == 0:
            continue
        assert float((a - b).norm()) / float(b.norm()) < 1e-4, name
    assert float((res["split"][2] - res["fp32"][2]).norm()) / float(res["fp32"][2].norm()) < 1e-4


def test_several_outstanding_forwards_each_own_their_activations():
    """Every autograd node owns the saved activations of its forward (parq_amd/decoder.py _Stash): a second forward before the
    first one's backward takes a workspace of its own, so (loss(dec(a)) + loss(dec(b))).backward() — gradient accumulation the
    way a reference user may write it — gives the sum of the two separate gradients, with dropout masks of the right forward
    (train mode, p = 0.1: a backward that regenerated the OTHER forward's masks would be off by tens of percent).  Once both
    backwards have run the module is back to one training workspace.  Eval-mode forwards differentiate too (dropout off)."""
    B, V, h, w, Q, dim = 1, 2, 8, 10, 16, 128
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=2, ffn=96, layers=2, dropout=0.1)
    W = synth.make_decoder_weights(cfg, 181)
    dec = make_decoder(cfg, W).train()
    a = scene_args(synth.make_scene(182, B, V, h, w, dim, smooth=True))
    b = scene_args(synth.make_scene(183, B, V, h, w, dim, smooth=True))
    f = lambda outs: sum(o["center_unnormalized"].sum() + o["ortho6d"].sum() for o in outs)
    torch.manual_seed(5)
    la, lb = f(dec(*a)), f(dec(*b))
    (la + lb).backward()
    both = {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None}
    dec.zero_grad(set_to_none=True)
    torch.manual_seed(5)                                           # the same two dropout seeds, one forward at a time
    f(dec(*a)).backward()
    f(dec(*b)).backward()
    ws_before = dec._train_ws
    for n, p in dec.named_parameters():
        if p.grad is not None and float(p.grad.norm()) > 0:
            assert float((both[n] - p.grad).norm()) <= 1e-4 * float(p.grad.norm()) + 1e-7, n
    f(dec(*a)).backward()
    assert dec._train_ws is ws_before                              # consumed stashes are reused, not re-allocated
    # eval mode under autograd: same graph, no dropout (the reference differentiates in eval mode, model/parq_decoder.py:134-163)
    dec.eval()
    dec.zero_grad(set_to_none=True)
    outs = dec(*a)
    assert outs[0]["ortho6d"].requires_grad
    f(outs).backward()
    g_eval = {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None}
    outs2 = dec(*a)                                                # deterministic: no dropout in eval mode
    assert torch.equal(outs[0]["ortho6d"].detach(), outs2[0]["ortho6d"].detach())
    with torch.no_grad():
        o_inf = dec(*a)                                            # the inference chain (folded position MLP): same numbers to rounding
    assert not o_inf[0]["ortho6d"].requires_grad
    assert float((o_inf[0]["ortho6d"] - outs[0]["ortho6d"].detach()).abs().max()) < 1e-4
    assert len(g_eval) >= 30
    # weight writes that bypass the version counter need invalidate_weights()
    dec.eval()
    with torch.no_grad():
        o1 = dec(*a)[0]["ortho6d"].clone()
        dec.refpoint.weight.data.add_(0.25)
        dec.invalidate_weights()
        o2 = dec(*a)[0]["ortho6d"]
    assert not torch.equal(o1, o2)


@pytest.mark.parametrize("heads", [4, 1])        # head dim 64 (the register-resident kernels) and 256 (the GEMM composition)
@pytest.mark.parametrize("mode,out_tol,grad_tol", [("fp16", 3e-4, 2e-2), ("bf16", 2e-3, 5e-2)])
def test_training_in_reduced_precision_attention_modes(mode, out_tol, grad_tol, heads):
    """BASELINE cfg 5 trains with fp16 cross-attention (cfg 2 names bf16): the training forward streams the single 16-bit K/V
    cache and the backward differentiates straight through the rounded K / V (fp32 values rebuilt from the cache).  Judged
    against float64 autograd of the oracle with the reduced-precision tolerances of the forward tests (operands rounded to
    2^-11 / 2^-8 relative): outputs 3e-4 / 2e-3, gradients Frobenius-relative 2e-2 / 5e-2 per tensor (measured: fp16 6.5e-3 / 7.3e-3, bf16 1.3e-2 / 2.6e-2 at head dim 64 / 256), dropout included in a
    second pass (finite, different from the dropout-free gradients)."""
    B, V, h, w, Q, dim, ffn, layers = 2, 2, 32, 41, 24, 256, 128, 3
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=heads, ffn=ffn, layers=layers, dropout=0.0)
    W = synth.make_decoder_weights(cfg, 571, damped=True)
    sc = synth.make_scene(572, B, V, h, w, dim, smooth=True)
    ncls = cfg.NUM_SEMCLS + 1
    cots = {"pred_logits": synth.normal(573, "cl", (layers, B, Q, ncls)), "center_unnormalized": synth.normal(574, "cc", (layers, B, Q, 3)),
            "size_unnormalized": synth.normal(575, "cs", (layers, B, Q, 3)), "ortho6d": synth.normal(576, "cr", (layers, B, Q, 6))}
    want, want_tok, oouts = oracle_grads(cfg, W, sc, cots)
    dec = make_decoder(cfg, W).train()
    dec.attention_mode = mode
    assert dec._train_mode() == mode
    outs = dec.forward_train(*scene_args(sc))
    for k in range(layers):
        for key in GKEYS:
            a, b = outs[k][key].cpu().numpy(), oouts[k][key].detach().numpy()
            assert np.abs(a - b).max() / max(1.0, np.abs(b).max()) < out_tol, (k, key)
    grads, d_tok = dec.backward({k: torch.from_numpy(v) for k, v in cots.items()})
    worst = {}
    for name, g in grads.items():
        if name in want:
            ref = want[name].numpy()
            worst[name] = np.linalg.norm(g.cpu().numpy().astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-9)
    print("\n%s training: worst gradient errors" % mode, sorted(worst.items(), key=lambda kv: -kv[1])[:4])
    assert max(worst.values()) < grad_tol, max(worst.values())
    rt = want_tok.numpy()
    terr = np.linalg.norm(d_tok.cpu().numpy().astype(np.float64) - rt) / np.linalg.norm(rt)
    print("token gradient error %.3e" % terr)
    assert terr < grad_tol
    assert not dec.fp16_range_exceeded()
    # with dropout (the reference trains with 0.1): the single-term dropout instantiation of the attention kernel
    cfg2 = synth.decoder_cfg(dim=dim, queries=Q, heads=heads, ffn=ffn, layers=layers, dropout=0.1)
    dec2 = make_decoder(cfg2, W).train()
    dec2.attention_mode = mode
    torch.manual_seed(3)
    dec2.forward_train(*scene_args(sc))
    g2, t2 = dec2.backward({k: torch.from_numpy(v) for k, v in cots.items()})
    assert all(torch.isfinite(v).all() for v in g2.values()) and torch.isfinite(t2).all()
    name = "parq_module.decoder.layers.0.multihead_attn.out_proj.weight"
    assert float((g2[name] - grads[name]).norm()) > 1e-3 * float(grads[name].norm())


def test_gradient_buckets_partition_the_arena_in_completion_order():
    """parq_grad_bucket (include/parq_hip.h): bucket 0 = what is final after phase 1 of the batched backward — cross out-proj, FFN,
    norm2 / norm3 and every head — bucket 1 = the front of the arena (reference points, position MLP, in-projections, self
    out-proj, norm1).  Every reference tensor lies in exactly one of the two contiguous ranges, the ranges are adjacent, and
    averaging them one after the other on ONE rank is the identity (world = 1 path of the bucketed all-reduce)."""
    import ctypes as C
    from parq_amd import _lib
    cfg = synth.decoder_cfg(dim=128, queries=16, heads=2, ffn=96, layers=2)
    dec = make_decoder(cfg, synth.make_decoder_weights(cfg, 191))
    lib, h = _lib.load(), dec._handle()
    off, cnt = C.c_int64(), C.c_int64()
    rng = []
    for b in (0, 1):
        _lib.check(lib.parq_grad_bucket(h, b, C.byref(off), C.byref(cnt)), "parq_grad_bucket")
        rng.append((off.value, cnt.value))
    (o0, n0), (o1, n1) = rng
    assert o1 == 0 and n1 > 0 and o0 == n1 and n0 > 0                     # late bucket in front, early bucket right behind it
    assert (o0 + n0) * 4 <= lib.parq_grad_arena_bytes(h)
    early = ("multihead_attn.out_proj", "linear1", "linear2", "norm2", "norm3", "mlp_heads.")
    o, r, c_, ld = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    seen = {0: 0, 1: 0}
    for name, p in dec._unique_params():
        if name.startswith("parq_module.decoder.norm."):
            continue
        _lib.check(lib.parq_arena_lookup(h, name.encode(), C.byref(o), C.byref(r), C.byref(c_), C.byref(ld)), name)
        first, last = o.value, o.value + (r.value - 1) * ld.value + c_.value
        in0 = o0 <= first and last <= o0 + n0
        in1 = o1 <= first and last <= o1 + n1
        assert in0 != in1, name
        assert in0 == any(k in name for k in early), (name, in0)
        seen[0 if in0 else 1] += 1
    assert seen[0] >= 20 and seen[1] >= 10, seen
    # unshared layers: one bucket (the layers interleave), still covering everything
    cfg2 = synth.decoder_cfg(dim=128, queries=16, heads=2, ffn=96, layers=2, share_weights=False)
    dec2 = make_decoder(cfg2, synth.make_decoder_weights(cfg2, 192))
    h2 = dec2._handle()
    _lib.check(lib.parq_grad_bucket(h2, 0, C.byref(off), C.byref(cnt)), "parq_grad_bucket")
    assert cnt.value == 0
    _lib.check(lib.parq_grad_bucket(h2, 1, C.byref(off), C.byref(cnt)), "parq_grad_bucket")
    assert off.value == 0 and cnt.value * 4 == lib.parq_grad_arena_bytes(h2)
