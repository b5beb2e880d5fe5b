"""Write tests/golden/g23_fpn_merge.npz: the reference's own FPN neck, ray-PE and tokenisation in float64 under its own autograd.

Development container only (it imports the reference tree through oracle.reference_loader; run from the repository root:
``python tools/make_golden_pyramid.py``).  Per case of tests/pyramid_cases.py:
  - the reference's ResnetFPN.forward (model/resnet_fpn.py:62-91), built with __new__ (torchvision is absent): its resnet_fpn is a
    stub returning the seeded levels '0'..'3' (float64 leaves), its transform the identity, freeze off;
  - the reference's AddRayPE + the composition of model/parq_lightning.py:72-85 on its output, loss = <cotangent, tokens>.
Stored: the token sample, the loss, the encoder-gradient summaries (oracle/make_golden.py grad_summary), a strided sample and the
norm / sum of every level gradient, and the camera_feature the neck produced.  Layout as g20 (a `meta` JSON of the cases).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pyramid_cases as PC  # noqa: E402
from oracle import make_golden as MG  # noqa: E402
from oracle import reference_loader  # noqa: E402


class _Stub(torch.nn.Module):
    def __init__(self, levels):
        super().__init__()
        self.levels = levels

    def forward(self, x):
        return {str(l): lv for l, lv in enumerate(self.levels)}


def run_case(ref, c):
    from einops import rearrange
    from model.resnet_fpn import ResnetFPN
    Wp, (cam, T_cp, T_wp, T_wl), levels, cot = PC.case_inputs(c)
    B, V = c["B"], c["V"]
    dbl = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    leaves = [dbl(lv).flatten(0, 1).requires_grad_(True) for lv in levels]
    neck = ResnetFPN.__new__(ResnetFPN)
    torch.nn.Module.__init__(neck)
    neck.resnet_fpn = _Stub(leaves)
    neck.layer = str(c["layer"])
    neck.transform = lambda x: x
    neck.freeze = False
    H, W = (np.array(c["sizes"][0]) * 4).tolist()
    batch = {"rgb_img": torch.zeros(B, V, 3, H, W, dtype=torch.float64), "camera": ref.Camera(dbl(cam))}
    batch = neck.forward(batch)
    pe = ref.AddRayPE(c["dim"], c["ray_points_scale"], 64, 0.25, 5.25).double()
    pe.load_state_dict({k: dbl(v) for k, v in Wp.items()}, strict=True)
    feats = batch["all_features"]
    enc = pe(feats, batch["camera_feature"], ref.Pose(dbl(T_cp)), ref.Pose(dbl(T_wp)), ref.Pose(dbl(T_wl)))
    tokens = rearrange(feats + enc, "b t c h w -> b (t h w) c")
    loss = (tokens * dbl(cot)).sum()
    loss.backward()
    p = c["name"] + "/"
    arrays = {p + "loss_value": np.float64(float(loss.detach())), p + "tokens_sample": tokens.detach().numpy()[:, ::11, ::7].copy(),
              p + "camera_feature": batch["camera_feature"]._data.detach().numpy().copy()}
    for name, prm in pe.named_parameters():
        for k, v in MG.grad_summary(prm.grad.numpy()).items():
            arrays[p + "grad/%s/%s" % (name, k)] = v
    for l, lv in enumerate(leaves):
        g = lv.grad.numpy().reshape(-1)
        arrays[p + "dlevel%d/norm" % l] = np.array([np.linalg.norm(g), g.sum()])
        arrays[p + "dlevel%d/sample" % l] = g[::PC.SAMPLE_STRIDE].copy()
    print("%s: loss %.6f, tokens %s" % (c["name"], float(loss.detach()), tuple(tokens.shape)))
    return arrays


def main():
    ref = reference_loader.load()
    arrays = {}
    for c in PC.CASES:
        arrays.update(run_case(ref, c))
    arrays["meta"] = np.frombuffer(json.dumps(PC.CASES, sort_keys=True).encode(), dtype=np.uint8)
    out = os.path.join(ROOT, "tests", "golden", PC.G23 + ".npz")
    np.savez_compressed(out, **arrays)
    print("wrote %s (%d arrays, %d bytes)" % (out, len(arrays), os.path.getsize(out)))


if __name__ == "__main__":
    main()
