"""ResnetFPN: the reference's 2-D backbone wrapper (model/resnet_fpn.py:16-91) around a user-supplied ResNet-FPN.

torchvision is not a dependency: pass the module itself, e.g. ``ResnetFPN(resnet_fpn_backbone("resnet50", ...), layer=0)`` — anything
that maps a (N, 3, H, W) image batch to an ordered dict with keys '0'..'3' (a fifth 'pool' level is ignored, as the reference's
``range(4)`` does).  It is held as ``self.resnet_fpn``, so a PARQ built with ``backbone2d=ResnetFPN(...)`` has the reference
checkpoint's ``backbone2d.resnet_fpn.*`` keys.

The neck's resize + concat (the reference's F.interpolate to level ``layer`` and torch.cat) is NOT done here: the batch carries the
four levels as they are (``fpn_features``, ``fpn_layer``) and PARQ.forward hands them to AddRayPE.tokens_from_pyramid, which
computes the resized features where the ray-PE kernel reads them (and whose backward has no float atomics, so a trainable backbone
works under torch.use_deterministic_algorithms(True), where torch's bilinear-interpolate backward raises).
"""
from __future__ import annotations

import torch
from torch import nn

from .wrappers import Camera, raw

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class ResnetFPN(nn.Module):
    def __init__(self, resnet_fpn: nn.Module, layer: int = 0, freeze: bool = False):
        super().__init__()
        layer = int(layer)
        if not 0 <= layer <= 3:
            raise ValueError("ResnetFPN: layer must be 0..3, got %d" % layer)
        self.resnet_fpn = resnet_fpn
        self.layer = layer
        self.freeze = bool(freeze)
        if self.freeze:
            # the reference calls self.feature_extractor.eval() here, an attribute it never defines; the backbone is meant
            self.resnet_fpn.eval()

    def forward(self, batch):
        """batch["rgb_img"] (B, T, 3, H, W) (or (B, 3, H, W): T = 1) -> batch with ``fpn_features`` (four (B, T, C_l, h_l, w_l)
        views of the backbone's levels '0'..'3'), ``fpn_layer`` and ``camera_feature`` = camera scaled by 1 / 2^(layer + 2)."""
        img = batch["rgb_img"]
        B = img.shape[0]
        T = img.shape[1] if img.dim() == 5 else 1
        x = img.flatten(0, 1) if img.dim() == 5 else img
        # torchvision.transforms.Normalize(mean, std) on a tensor: (x - mean) / std per channel
        mean = torch.tensor(IMAGENET_MEAN, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        std = torch.tensor(IMAGENET_STD, dtype=x.dtype, device=x.device).view(-1, 1, 1)
        x = (x - mean) / std
        if self.freeze:
            with torch.no_grad():
                feats = self.resnet_fpn(x)
        else:
            feats = self.resnet_fpn(x)
        missing = [k for k in ("0", "1", "2", "3") if k not in feats]
        if missing:
            raise KeyError("ResnetFPN: the backbone's output has no level(s) %s (expected an ordered dict with '0'..'3')" % missing)
        batch["fpn_features"] = [feats[str(l)].unflatten(0, (B, T)) for l in range(4)]
        batch["fpn_layer"] = self.layer
        cam = batch["camera"]
        scaled = (cam if isinstance(cam, Camera) else Camera(raw(cam))).scale(1 / 2 ** (self.layer + 2))
        batch["camera_feature"] = scaled if hasattr(cam, "_data") else raw(scaled)
        return batch
