"""Inputs of the g23 fixture (tests/golden/g23_fpn_merge.npz, written by tools/make_golden_pyramid.py): the reference's FPN neck
(model/resnet_fpn.py:62-91) + AddRayPE + tokenisation (model/parq_lightning.py:72-85), regenerated here from the seeds."""
import numpy as np

from parq_amd import synth

G23 = "g23_fpn_merge"
SAMPLE_STRIDE = 17              # level-gradient samples: every 17th element of the flattened (B, T, C/4, h_l, w_l) gradient

CASES = [
    # torchvision-style ceil sizes of a 120x160 image (strides 4, 8, 16, 32), target level 0: every other level is upsampled
    dict(name="d256_l0", dim=256, layer=0, sizes=[[30, 40], [15, 20], [8, 10], [4, 5]], B=1, V=2, seed=231, gseed=232, lseed=233,
         cseed=234, ray_points_scale=[-2.0, 2.0, -1.5, 0.0, 0.25, 4.25]),
    # odd sizes, target level 1: level 0 is DOWNsampled (27x35 -> 13x17), levels 2 and 3 upsampled by non-integer ratios
    dict(name="d128_l1", dim=128, layer=1, sizes=[[27, 35], [13, 17], [7, 9], [4, 5]], B=1, V=2, seed=241, gseed=242, lseed=243,
         cseed=244, ray_points_scale=[-3.0, 3.0, -2.0, 0.5, 0.25, 5.25]),
]


def case_inputs(c):
    """(encoder weights, (camera at the IMAGE resolution, T_cp, T_wp, T_wl), four levels (B, V, C/4, h_l, w_l), cotangent)."""
    B, V, C, layer = c["B"], c["V"], c["dim"], c["layer"]
    h, w = c["sizes"][layer]
    Wp = synth.make_ray_pe_weights(C, c["seed"])
    cam, T_cp, T_wp, T_wl = synth.make_geometry(c["gseed"], B, V, h, w)
    # the image the backbone saw is 2^(layer + 2) times the target level: the camera ResnetFPN scales down (c' = (c + 0.5) s - 0.5)
    s = 2.0 ** (layer + 2)
    cam = np.asarray(cam, np.float64).copy()
    cam[..., 0:4] *= s
    cam[..., 4:6] = (cam[..., 4:6] + 0.5) * s - 0.5
    levels = [synth.normal(c["lseed"] + l, "level%d" % l, (B, V, C // 4, hl, wl), std=0.5) for l, (hl, wl) in enumerate(c["sizes"])]
    cot = synth.normal(c["cseed"], "cot", (B, V * h * w, C))
    return Wp, (cam, T_cp, T_wp, T_wl), levels, cot
