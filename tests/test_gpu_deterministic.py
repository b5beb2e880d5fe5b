"""GPU tier: deterministic mode (include/parq_hip.h parq_set_deterministic, PARQ_RAYPE_BWD_DETERMINISTIC, PARQ_SETLOSS_DETERMINISTIC).

Under torch.use_deterministic_algorithms(True) a whole PARQ.training_step + backward — ray-PE node, decoder forward and backward
with dropout, set loss — must give the same bits on every run: every parameter gradient, the feature gradient and the loss.  The
geometries make the former float atomics contend (many queries per token, many row ranges per weight gradient)."""
import os
import subprocess
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from parq_amd import PARQ, Camera, Obb3D, Pose, synth  # noqa: E402

pytestmark = pytest.mark.gpu

# B, V, h, w, dim, heads, queries, ffn, iterations
GEO_CONTEND = (2, 10, 60, 80, 256, 4, 256, 512, 8)
GEO_SHIPPED = (1, 3, 60, 80, 1024, 4, 256, 1024, 4)      # the reference's shipped width: 4 heads of 256, C = 1024 dW


def _setup(geo, seed=11):
    B, V, h, w, Cd, H, Qn, F, I = geo
    dcfg = synth.decoder_cfg(dim=Cd, queries=Qn, heads=H, ffn=F, layers=I, dropout=0.1)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg), OPTIMIZER=NS(LEARNING_RATE=1e-4, AUTOSCALE_LR=False))
    torch.manual_seed(seed)
    model = PARQ(cfg).cuda().train()
    cam, T_cp, T_wp, T_wl = synth.make_geometry(seed + 1, B, V, h, w)
    obbs, sym = synth.make_boxes(seed + 2, B, 6, max_box=10)
    to = lambda a: torch.from_numpy(a).cuda()
    feats = to(synth.normal(seed + 3, "f", (B, V, Cd, h, w), std=0.5)).requires_grad_(True)
    batch = {"all_features": feats, "camera_feature": Camera(to(cam)), "T_camera_pseudoCam": Pose(to(T_cp)),
             "T_world_pseudoCam": Pose(to(T_wp)), "T_world_local": Pose(to(T_wl)), "obbs_padded": Obb3D(to(obbs)), "sym": to(sym)}
    return model, batch


def _step(model, batch, seed=5):
    """One training step from fixed seeds: {name: tensor} of the loss, every parameter gradient and the feature gradient."""
    np.random.seed(seed)                                    # the matcher's np.random.choice cap
    torch.manual_seed(seed)                                 # the dropout seed of the forward
    model.zero_grad(set_to_none=True)
    batch["all_features"].grad = None
    loss = model.training_step(batch, 0)
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach().clone(), "features.grad": batch["all_features"].grad.clone()}
    out.update({n + ".grad": p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    return out


def _differing(a, b):
    assert a.keys() == b.keys()
    return sorted(k for k in a if not torch.equal(a[k], b[k]))


@pytest.fixture
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev)


@pytest.mark.parametrize("geo", [GEO_CONTEND, GEO_SHIPPED], ids=["contend", "shipped"])
def test_training_step_repeats_bitwise(deterministic, geo):
    model, batch = _setup(geo)
    runs = [_step(model, batch) for _ in range(3)]
    assert len(runs[0]) > 40
    assert all(torch.isfinite(t).all() for t in runs[0].values())
    for r in runs[1:]:
        assert _differing(runs[0], r) == []


def test_training_step_bits_under_concurrent_inference(deterministic):
    model, batch = _setup(GEO_CONTEND)
    ref = _step(model, batch)
    # a second decoder runs inference forwards on another stream while the step repeats
    other, _ = _setup(GEO_CONTEND, seed=21)
    dec = other.box3d_decoder.eval()
    side = torch.cuda.Stream()
    cam, T_cp, T_wp, T_wl = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
                             for a in synth.make_geometry(22, 2, 10, 60, 80))
    tokens = torch.randn(2, 10 * 60 * 80, 256, device="cuda")
    torch.cuda.synchronize()
    with torch.no_grad(), torch.cuda.stream(side):
        for _ in range(3):
            dec(tokens, cam, T_cp, T_wp, T_wl, feat_hw=(60, 80))
    got = _step(model, batch)
    torch.cuda.synchronize()
    assert _differing(ref, got) == []


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import test_gpu_deterministic as t
torch.use_deterministic_algorithms(True)
m, b = t._setup(t.GEO_CONTEND)
torch.save({k: v.cpu() for k, v in t._step(m, b).items()}, sys.argv[2])
"""


def test_training_step_bits_in_fresh_process(deterministic, tmp_path):
    model, batch = _setup(GEO_CONTEND)
    ref = {k: v.cpu() for k, v in _step(model, batch).items()}
    out = tmp_path / "grads.pt"
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(__file__), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _differing(ref, torch.load(out)) == []


def _adamw_run(steps=5):
    model, batch = _setup(GEO_CONTEND)
    batch["all_features"].requires_grad_(False)
    opt = model.configure_optimizers()
    losses = []
    for it in range(steps):
        np.random.seed(100 + it)
        torch.manual_seed(100 + it)
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, it)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return losses, {n: p.detach().clone() for n, p in model.named_parameters()}


def test_adamw_training_run_repeats_bitwise(deterministic):
    l1, p1 = _adamw_run()
    l2, p2 = _adamw_run()
    assert all(torch.equal(a, b) for a, b in zip(l1, l2))
    assert _differing(p1, p2) == []


@pytest.mark.parametrize("geo", [GEO_CONTEND, GEO_SHIPPED], ids=["contend", "shipped"])
def test_deterministic_gradients_match_default_mode(geo):
    """The fixed-order forms compute the same gradients as the default kernels up to fp32 summation order (the default path is
    held to the float64 oracle by test_gpu_backward.py): Frobenius-relative < 2e-3, max-norm-relative < 2e-2 per tensor."""
    prev = torch.are_deterministic_algorithms_enabled()
    model, batch = _setup(geo)
    try:
        torch.use_deterministic_algorithms(False)
        base = _step(model, batch)
        torch.use_deterministic_algorithms(True)
        det = _step(model, batch)
    finally:
        torch.use_deterministic_algorithms(prev)
    assert abs(float(base["loss"]) - float(det["loss"])) <= 1e-4 * max(1.0, abs(float(base["loss"])))
    for k in base:
        a, b = base[k].double(), det[k].double()
        scale = float(a.norm())
        if scale == 0.0:
            assert float(b.abs().max()) == 0.0, k
            continue
        assert float((a - b).norm()) / scale < 2e-3, k
        assert float((a - b).abs().max()) / float(a.abs().max()) < 2e-2, k
