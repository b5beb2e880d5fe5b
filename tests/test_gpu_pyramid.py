"""GPU tier: the FPN neck fused into the ray-PE tokenisation (AddRayPE.tokens_from_pyramid, parq_ray_pe_fpn, parq_fpn_backward).

The yardstick is the composition the reference runs (model/resnet_fpn.py:76-84 + parq_lightning.py:72-85): every level resized to
level `layer` with F.interpolate(mode="bilinear"), concatenated, then AddRayPE.tokens.  The target level's channel block must be
bit-identical to it (the kernels add the same value at the same place), the resized blocks within fp32 rounding of torch's own
interpolate, and everything bit-identical where every bilinear weight and product is exact."""
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
from parq_amd import PARQ, AddRayPE, Camera, InFlight, Obb3D, Pose, ResnetFPN, synth  # noqa: E402

pytestmark = pytest.mark.gpu

LAYER0 = ((60, 80), (30, 40), (15, 20), (8, 10))          # torchvision-style ceil sizes; 8x10 -> 60x80 is a 7.5 ratio
LAYER1 = ((60, 80), (30, 40), (15, 20), (8, 10))          # layer 1: level 0 is downsampled 2x, level 3 upsampled 3.75x
ODD = ((37, 51), (19, 26), (10, 13), (5, 7))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _geometry(seed, B, V, h, w):
    cam, T_cp, T_wp, T_wl = synth.make_geometry(seed, B, V, h, w)
    return Camera(_dev(cam)), Pose(_dev(T_cp)), Pose(_dev(T_wp)), Pose(_dev(T_wl))


def _module(C, seed):
    torch.manual_seed(seed)
    m = AddRayPE(C).cuda()
    with torch.no_grad():                                   # encoder scale of trained weights: tokens of O(1)
        for p in m.parameters():
            p.mul_(0.5)
    return m


def _levels(seed, B, V, cl, sizes, dyadic=False):
    g = torch.Generator().manual_seed(seed)
    out = []
    for (h, w) in sizes:
        if dyadic:
            x = torch.randint(-64, 65, (B, V, cl, h, w), generator=g).float() / 64.0
        else:
            x = torch.randn(B, V, cl, h, w, generator=g) * 0.5
        out.append(x.cuda())
    return out


def _compose(levels, layer):
    """The reference neck: F.interpolate to level `layer`'s size (align_corners=False) + cat along the channels."""
    B, V = levels[0].shape[:2]
    size = tuple(levels[layer].shape[-2:])
    return torch.cat([F.interpolate(lv.flatten(0, 1), size, mode="bilinear").unflatten(0, (B, V)) for lv in levels], 2)


@pytest.mark.parametrize("C", [256, 1024, 128])
@pytest.mark.parametrize("layer,sizes", [(0, LAYER0), (1, LAYER1), (0, ODD), (2, ODD)], ids=["l0", "l1", "odd-l0", "odd-l2"])
def test_parity_with_the_torch_composition(C, layer, sizes):
    B, V = 1, 3
    h, w = sizes[layer]
    mod = _module(C, 3).eval()
    geo = _geometry(5, B, V, h, w)
    levels = _levels(7, B, V, C // 4, sizes)
    with torch.no_grad():
        got = mod.tokens_from_pyramid(levels, layer, *geo)
        want = mod.tokens(_compose(levels, layer), *geo)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (B, V * h * w, C) and got.dtype == torch.float32
    cl = C // 4
    for l in range(4):
        a, b = got[..., l * cl:(l + 1) * cl], want[..., l * cl:(l + 1) * cl]
        if l == layer:
            assert torch.equal(a, b), ("target level", l)
        else:
            err = ((a - b).abs() / b.abs().clamp_min(1.0)).max().item()
            assert err <= 2e-6, (l, err)


@pytest.mark.parametrize("C", [256, 1024])
def test_exact_weights_give_identical_tokens_and_decoder_outputs(C):
    """Dyadic level values (k/64) and integer ratios 2 and 4: every bilinear weight and product is exact, so the fused gather and
    torch's interpolate + cat hand the kernels the same features — tokens and all decoder outputs of PARQ.forward are bit-identical."""
    B, V, layer = 1, 2, 0
    sizes = ((32, 40), (16, 20), (8, 10), (8, 10))
    h, w = sizes[layer]
    dcfg = synth.decoder_cfg(dim=C, queries=64, heads=4, ffn=256, layers=2)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=C, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25,
                                   MAX_DEPTH=5.25), DECODER=dcfg))
    torch.manual_seed(13)
    model = PARQ(cfg).cuda().eval()
    model.box3d_decoder.range_check = "off"
    cam, T_cp, T_wp, T_wl = _geometry(15, B, V, h, w)
    levels = _levels(17, B, V, C // 4, sizes, dyadic=True)
    base = {"camera_feature": cam, "T_camera_pseudoCam": T_cp, "T_world_pseudoCam": T_wp, "T_world_local": T_wl}
    with torch.no_grad():
        tok = model.add_ray_pe.tokens_from_pyramid(levels, layer, cam, T_cp, T_wp, T_wl)
        ref = model.add_ray_pe.tokens(_compose(levels, layer), cam, T_cp, T_wp, T_wl)
        assert torch.equal(tok, ref)
        _, got = model(dict(base, fpn_features=levels, fpn_layer=layer), 0)
        got = [{k: v.clone() for k, v in o.items()} for o in got]
        _, want = model(dict(base, all_features=_compose(levels, layer)), 0)
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        for key in b:
            assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("C", [256, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16bit_rows_are_the_rounded_fp32_rows(C, dtype):
    B, V, layer = 1, 3, 1
    h, w = LAYER1[layer]
    mod = _module(C, 21).eval()
    geo = _geometry(22, B, V, h, w)
    levels = _levels(23, B, V, C // 4, LAYER1)
    with torch.no_grad():
        full = mod.tokens_from_pyramid(levels, layer, *geo)
        half = mod.tokens_from_pyramid(levels, layer, *geo, dtype=dtype)
    torch.cuda.synchronize()
    assert half.dtype == dtype
    assert torch.equal(half.view(torch.int16), full.to(dtype).view(torch.int16))


def _relfro(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("C", [256, 1024])
@pytest.mark.parametrize("layer,sizes", [(0, LAYER0), (1, ODD)], ids=["l0", "odd-l1"])
def test_backward_matches_torch_autograd_of_the_composition(C, layer, sizes):
    B, V = 2, 2
    h, w = sizes[layer]
    mod = _module(C, 31).train()
    geo = _geometry(32, B, V, h, w)
    base = _levels(33, B, V, C // 4, sizes)
    cot = torch.randn(B, V * h * w, C, generator=torch.Generator().manual_seed(34)).cuda()

    def run(fused):
        mod.zero_grad(set_to_none=True)
        lv = [x.clone().requires_grad_(True) for x in base]
        tok = mod.tokens_from_pyramid(lv, layer, *geo) if fused else mod.tokens(_compose(lv, layer), *geo)
        (tok * cot).sum().backward()
        torch.cuda.synchronize()
        return [x.grad for x in lv], {n: p.grad.clone() for n, p in mod.named_parameters()}

    lg, eg = run(True)
    lr, er = run(False)
    for l in range(4):
        assert lg[l].shape == base[l].shape
        assert _relfro(lg[l], lr[l]) <= 1e-5, (l, _relfro(lg[l], lr[l]))
    for n in er:
        assert _relfro(eg[n], er[n]) <= 1e-5, (n, _relfro(eg[n], er[n]))


def test_level_gradients_repeat_bitwise_and_only_requested_ones_are_returned():
    B, V, C, layer = 1, 3, 256, 1
    h, w = LAYER1[layer]
    mod = _module(C, 41).train()
    geo = _geometry(42, B, V, h, w)
    base = _levels(43, B, V, C // 4, LAYER1)
    cot = torch.randn(B, V * h * w, C, generator=torch.Generator().manual_seed(44)).cuda()
    grads = []
    for _ in range(2):
        lv = [x.clone().requires_grad_(i != 2) for i, x in enumerate(base)]
        (mod.tokens_from_pyramid(lv, layer, *geo) * cot).sum().backward()
        grads.append([x.grad for x in lv])
    torch.cuda.synchronize()
    assert grads[0][2] is None
    for a, b in zip(grads[0], grads[1]):
        assert (a is None and b is None) or torch.equal(a, b)


# ---- deterministic mode: test_gpu_deterministic.py's geometries with fpn_features leaves that require grad
GEO_CONTEND = (2, 10, 60, 80, 256, 4, 256, 512, 8)
GEO_SHIPPED = (1, 3, 60, 80, 1024, 4, 256, 1024, 4)


def _train_setup(geo, seed=11):
    B, V, h, w, Cd, H, Qn, Fd, I = geo
    dcfg = synth.decoder_cfg(dim=Cd, queries=Qn, heads=H, ffn=Fd, layers=I, dropout=0.1)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg), OPTIMIZER=NS(LEARNING_RATE=1e-4, AUTOSCALE_LR=False))
    torch.manual_seed(seed)
    model = PARQ(cfg).cuda().train()
    cam, T_cp, T_wp, T_wl = synth.make_geometry(seed + 1, B, V, h, w)
    obbs, sym = synth.make_boxes(seed + 2, B, 6, max_box=10)
    levels = [x.requires_grad_(True) for x in _levels(seed + 3, B, V, Cd // 4, LAYER0)]
    batch = {"fpn_features": levels, "fpn_layer": 0, "camera_feature": Camera(_dev(cam)), "T_camera_pseudoCam": Pose(_dev(T_cp)),
             "T_world_pseudoCam": Pose(_dev(T_wp)), "T_world_local": Pose(_dev(T_wl)), "obbs_padded": Obb3D(_dev(obbs)),
             "sym": _dev(sym)}
    return model, batch


def _train_step(model, batch, seed=5):
    np.random.seed(seed)
    torch.manual_seed(seed)
    model.zero_grad(set_to_none=True)
    for lv in batch["fpn_features"]:
        lv.grad = None
    loss = model.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach().clone()}
    out.update({"level%d.grad" % i: lv.grad.clone() for i, lv in enumerate(batch["fpn_features"])})
    out.update({n + ".grad": p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    return out


def _level_grads_for(mod, levels, layer, geo, cot):
    lv = [x.detach().clone().requires_grad_(True) for x in levels]
    mod.tokens_from_pyramid(lv, layer, *geo).backward(cot)
    torch.cuda.synchronize()
    return [x.grad for x in lv]


@pytest.mark.parametrize("geo", [GEO_CONTEND, GEO_SHIPPED], ids=["contend", "shipped"])
def test_deterministic_training_step_through_a_pyramid(geo):
    """Under torch.use_deterministic_algorithms(True) two PARQ.training_step + backward runs give the same bits for the loss, every
    parameter gradient and every level gradient.  For the same d tokens the level gradients are the default mode's bits (the
    adjoint has one form; what differs between the modes upstream is the decoder's d tokens)."""
    model, batch = _train_setup(geo)
    B, V, h, w, Cd = geo[:5]
    cot = torch.randn(B, V * h * w, Cd, generator=torch.Generator().manual_seed(9)).cuda()
    geo4 = tuple(batch[k] for k in ("camera_feature", "T_camera_pseudoCam", "T_world_pseudoCam", "T_world_local"))
    default = _level_grads_for(model.add_ray_pe, batch["fpn_features"], 0, geo4, cot)
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = [_train_step(model, batch) for _ in range(2)]
        det = _level_grads_for(model.add_ray_pe, batch["fpn_features"], 0, geo4, cot)
        # the torch composition: raises where upsample_bilinear2d's CUDA backward has no deterministic form
        lv = [x.detach().clone().requires_grad_(True) for x in batch["fpn_features"]]
        raised = False
        try:
            _compose(lv, 0).sum().backward()
        except RuntimeError:
            raised = True
    finally:
        torch.use_deterministic_algorithms(prev)
    assert len(runs[0]) > 40
    assert all(torch.isfinite(t).all() for t in runs[0].values())
    differ = sorted(k for k in runs[0] if not torch.equal(runs[0][k], runs[1][k]))
    assert differ == []
    for i in range(4):
        assert torch.equal(det[i], default[i]), i
    # torch releases whose bilinear-interpolate CUDA backward has no deterministic form raise there; releases that route it through
    # a deterministic decomposition do not, and then there is nothing to assert about the composition
    print("torch %s: composition under deterministic mode %s" % (torch.__version__, "raises" if raised else "runs"))


def test_inference_call_allocates_only_its_tokens():
    """Shipped geometry (3 views, 60x80, 4 x 256 channels): no resized stack, no temporaries beyond the token output."""
    B, V, C, layer = 1, 3, 1024, 0
    h, w = LAYER0[layer]
    mod = _module(C, 51).eval()
    geo = _geometry(52, B, V, h, w)
    levels = _levels(53, B, V, C // 4, LAYER0)
    with torch.no_grad():
        mod.tokens_from_pyramid(levels, layer, *geo)           # warm-up: workspace, weight copies
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = mod.tokens_from_pyramid(levels, layer, *geo)
        torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert peak - before <= out.numel() * 4 + (1 << 20), (peak - before, out.numel() * 4)


def test_in_flight_forwards_over_pyramid_batches_are_the_serial_ones():
    B, V, C, layer = 1, 3, 256, 0
    h, w = LAYER0[layer]
    dcfg = synth.decoder_cfg(dim=C, queries=64, heads=4, ffn=256, layers=2)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=C, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25,
                                   MAX_DEPTH=5.25), DECODER=dcfg))
    torch.manual_seed(61)
    model = PARQ(cfg).cuda().eval()
    model.box3d_decoder.range_check = "off"

    def batch(seed):
        cam, T_cp, T_wp, T_wl = _geometry(seed, B, V, h, w)
        return {"fpn_features": _levels(seed + 1, B, V, C // 4, LAYER0), "fpn_layer": layer, "camera_feature": cam,
                "T_camera_pseudoCam": T_cp, "T_world_pseudoCam": T_wp, "T_world_local": T_wl}
    batches = [batch(70 + 10 * i) for i in range(3)]
    with torch.no_grad():
        want = []
        for b in batches:
            _, outs = model(dict(b), 0)
            want.append([{k: v.clone() for k, v in o.items()} for o in outs])
        torch.cuda.synchronize()
        runner = InFlight(model, depth=2)
        for rep in range(2):
            tickets = [runner.submit(dict(b), 0) for b in batches]
            got = [t.result()[1] for t in tickets]
            torch.cuda.synchronize()
            for i in range(3):
                for k in range(len(want[i])):
                    for key in want[i][k]:
                        assert torch.equal(got[i][k][key], want[i][k][key]), (rep, i, k, key)


class _ConvPyramid(torch.nn.Module):
    """A small stand-in for a ResNet-FPN: strided convs, an ordered dict of four levels (and a 'pool' level that is ignored)."""

    def __init__(self, cl):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, cl, 3, stride=4, padding=1)
        self.down = torch.nn.ModuleList([torch.nn.Conv2d(cl, cl, 3, stride=2, padding=1) for _ in range(3)])

    def forward(self, x):
        f = [torch.relu(self.stem(x))]
        for d in self.down:
            f.append(torch.relu(d(f[-1])))
        return {"0": f[0], "1": f[1], "2": f[2], "3": f[3], "pool": F.max_pool2d(f[3], 1, 2)}


class _ComposeBackbone(torch.nn.Module):
    """The same backbone with the reference's neck in torch (interpolate + cat -> all_features)."""

    def __init__(self, fpn, layer):
        super().__init__()
        self.fpn, self.layer = fpn, layer

    def forward(self, batch):
        b = self.fpn(dict(batch))
        batch["all_features"] = _compose(b["fpn_features"], self.layer)
        batch["camera_feature"] = b["camera_feature"]
        return batch


@pytest.mark.parametrize("layer", [0, 1])
def test_training_step_through_resnet_fpn_matches_the_composition(layer):
    B, V, C = 1, 2, 256
    H, W = 160, 224
    dcfg = synth.decoder_cfg(dim=C, queries=64, heads=4, ffn=256, layers=2)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=C, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25,
                                   MAX_DEPTH=5.25), DECODER=dcfg))
    torch.manual_seed(81)
    conv = _ConvPyramid(C // 4)
    fpn = ResnetFPN(conv, layer=layer)
    model = PARQ(cfg, backbone2d=fpn).cuda().train()
    cam, T_cp, T_wp, T_wl = synth.make_geometry(82, B, V, H, W)
    obbs, sym = synth.make_boxes(83, B, 6, max_box=10)
    img = torch.rand(B, V, 3, H, W, generator=torch.Generator().manual_seed(84)).cuda()
    batch = {"rgb_img": img, "camera": Camera(_dev(cam)), "T_camera_pseudoCam": Pose(_dev(T_cp)), "T_world_pseudoCam": Pose(_dev(T_wp)),
             "T_world_local": Pose(_dev(T_wl)), "obbs_padded": Obb3D(_dev(obbs)), "sym": _dev(sym)}

    def step():
        np.random.seed(5)
        torch.manual_seed(5)
        model.zero_grad(set_to_none=True)
        loss = model.training_step(dict(batch), 0)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in conv.named_parameters()}

    loss_f, g_f = step()
    model.backbone2d = _ComposeBackbone(fpn, layer)
    loss_c, g_c = step()
    assert abs(loss_f.item() - loss_c.item()) <= 1e-5 * max(1.0, abs(loss_c.item()))
    assert g_f.keys() == g_c.keys() and len(g_f) == 8
    for n in g_c:
        err = ((g_f[n] - g_c[n]).abs().max() / g_c[n].abs().max().clamp_min(1e-30)).item()
        assert err <= 1e-5, (n, err)


@pytest.mark.parametrize("case", [0, 1], ids=["d256_l0", "d128_l1"])
def test_g23_pin_against_the_reference_float64_autograd(case):
    """g23: the reference's own ResnetFPN neck + AddRayPE + tokenisation under float64 autograd.  tokens_from_pyramid as an
    autograd node (eval mode, like the fixture): token sample 2e-5, encoder gradients 1e-4 Frobenius, level gradients 1e-6 (target
    level) / 1e-5 (resized levels, the bound torch's own fp32 interpolate meets)."""
    import json
    import pyramid_cases as PC
    from oracle import make_golden as MG
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", PC.G23 + ".npz"))
    assert json.loads(bytes(z["meta"]).decode()) == PC.CASES
    c = PC.CASES[case]
    p = c["name"] + "/"
    Wp, (_, T_cp, T_wp, T_wl), levels, cot = PC.case_inputs(c)
    pe = AddRayPE(c["dim"], c["ray_points_scale"], 64, 0.25, 5.25)
    pe.load_state_dict({k: torch.from_numpy(v) for k, v in Wp.items()}, strict=True)
    pe = pe.cuda().eval()
    lv = [_dev(x).requires_grad_(True) for x in levels]
    tok = pe.tokens_from_pyramid(lv, c["layer"], Camera(_dev(z[p + "camera_feature"])), Pose(_dev(T_cp)), Pose(_dev(T_wp)),
                                 Pose(_dev(T_wl)))
    assert tok.requires_grad
    assert np.abs(tok.detach().cpu().numpy()[:, ::11, ::7] - z[p + "tokens_sample"]).max() < 2e-5
    (tok * _dev(cot)).sum().backward()
    for name, prm in pe.named_parameters():
        g = prm.grad.cpu().numpy().astype(np.float64).reshape(-1)
        if p + "grad/%s/full" % name in z.files:
            ref = z[p + "grad/%s/full" % name]
            err = np.linalg.norm(g - ref) / np.linalg.norm(ref)
        else:
            ref = z[p + "grad/%s/sample" % name]
            err = max(np.linalg.norm(g[::MG.GRAD_STRIDE] - ref) / np.linalg.norm(ref),
                      abs(np.linalg.norm(g) - z[p + "grad/%s/norm" % name][0]) / z[p + "grad/%s/norm" % name][0])
        assert err < 1e-4, (name, err)
    # the target level's gradient is a transpose of d tokens: 1e-6.  The resized levels use torch's fp32 bilinear weights (as the
    # forward must); their rounding against the float64 weights (half an ulp of the source coordinate, ~1e-6 at 25 texels) puts
    # torch's own fp32 F.interpolate backward 4e-6 from this fixture too, so those are held to 1e-5
    for l, x in enumerate(lv):
        d = x.grad.cpu().numpy().astype(np.float64).reshape(-1)
        err = np.abs(d[::PC.SAMPLE_STRIDE] - z[p + "dlevel%d/sample" % l]).max()
        assert err < (1e-6 if l == c["layer"] else 1e-5), (l, err)
