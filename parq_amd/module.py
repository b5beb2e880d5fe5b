"""PARQ: the reference Lightning module's interface (model/parq_lightning.py:28-145) over the HIP path.

``forward(batch, batch_idx) -> (losses, outputs)`` reproduces model/parq_lightning.py:68-95 for the part
that is in scope this round: ray positional encoding + tokenisation + decoder.  The 2-D backbone is not
part of the decoder path (torchvision ResNet-FPN): pass any callable that adds
``all_features`` (B,T,C,h,w) and ``camera_feature`` to the batch, or feed batches that already carry them.
``backbone2d=parq_amd.ResnetFPN(resnet_fpn)`` adds the four FPN levels instead (``fpn_features``, ``fpn_layer``): their
resize + concat is fused into the tokenisation (AddRayPE.tokens_from_pyramid).
Lightning is used as the base class only when it is importable (it is not on the GPU image).
"""
from __future__ import annotations

import math

import torch
from torch import nn

from .decoder import PARQDecoder
from .ray_pe import AddRayPE

try:                                                    # pragma: no cover - absent on the target image
    from pytorch_lightning import LightningModule as _Base
except Exception:                                       # noqa: BLE001
    _Base = nn.Module


def _get(cfg, path):
    for k in path.split("."):
        cfg = cfg[k] if isinstance(cfg, dict) else getattr(cfg, k)
    return cfg


class PARQ(_Base):
    def __init__(self, cfg, backbone2d=None):
        super().__init__()
        self.cfg = cfg
        self.backbone2d = backbone2d
        tk = _get(cfg, "MODEL.TOKENIZER")
        self.add_ray_pe = AddRayPE(_get(tk, "OUT_CHANNELS"), _get(tk, "RAY_POINTS_SCALE"), _get(tk, "NUM_SAMPLES"),
                                   _get(tk, "MIN_DEPTH"), _get(tk, "MAX_DEPTH"))
        self.box3d_decoder = PARQDecoder(_get(cfg, "MODEL.DECODER"))
        self.for_vis = _get(cfg, "MODEL.DECODER.FOR_VIS")
        # None: float32 tokens (the reference).  torch.float16 / torch.bfloat16: the inference chain hands the decoder 16-bit tokens
        # written by the ray-PE kernel, which the decoder reads as they are (bit-identical to decoding their float32 upcast); with a
        # graph the ray-PE node stays float32 and its output is converted (the node emitting 16-bit tokens itself is out of scope:
        # its 16-bit output needs the no-hidden flag), and the decoder's autograd path reads the 16-bit tokens as they are too — no
        # float32 copy of the tokens lives from the forward to the backward
        self.token_dtype = None
        self.synced_metrics = {}          # validation metrics averaged over the ranks (what the reference logs with sync_dist=True)

    @property
    def batch_invariant(self):
        """Batch-invariant inference of the decoder (``PARQDecoder.batch_invariant``): a scene's outputs — hence its detections —
        do not depend on how many scenes share the call.  The ray-PE tokenisation and ``parse_pred`` work scene by scene as they are."""
        return self.box3d_decoder.batch_invariant

    @batch_invariant.setter
    def batch_invariant(self, on):
        self.box3d_decoder.batch_invariant = bool(on)

    @property
    def match_on_device(self):
        """The decoder's training loss matches predictions to boxes on the device (``PARQDecoder.match_on_device``; the draw of a
        capped neighbourhood is then keyed by ``box3d_decoder.match_seed`` and the decoder's step counter)."""
        return self.box3d_decoder.match_on_device

    @match_on_device.setter
    def match_on_device(self, on):
        self.box3d_decoder.match_on_device = bool(on)

    def view_window(self, B, V, h, w, T_world_local):
        """A streaming window of V view slots (parq_amd.ViewWindow) that also encodes: ``win.put_features(slot, features or
        (levels, layer), camera, T_camera_pseudoCam, T_world_pseudoCam)`` tokenises the put views only, with the window's
        ``T_world_local`` and in ``token_dtype``; ``win.forward()`` equals ``forward(batch)[1]`` on the assembled batch."""
        from .view_window import FeatureViewWindow
        return FeatureViewWindow(self, B, V, h, w, T_world_local)

    def set_data_parallel(self, on=True):
        """One process per GPU, scenes sharded (train.py:103-108 runs DDP): with ``on`` every trainable tensor of the module —
        the decoder's flat gradient arena and the ray-PE encoder's four tensors — is averaged over the default process group
        (RCCL over xGMI) inside the two backward nodes, i.e. two collectives per step instead of DDP's per-tensor buckets.
        Do not wrap the module in DistributedDataParallel as well."""
        self.box3d_decoder.dp_all_reduce = bool(on)
        self.add_ray_pe.dp_all_reduce = bool(on)
        return self

    def forward(self, batch, batch_idx=0):
        if self.backbone2d is not None:
            batch = self.backbone2d(batch)
        if "fpn_features" in batch:
            # ResnetFPN's four levels: the neck's resize + concat (model/resnet_fpn.py:62-91) fused into the tokenisation
            levels, layer = batch["fpn_features"], batch["fpn_layer"]
            input_tokens = self.add_ray_pe.tokens_from_pyramid(levels, layer, batch["camera_feature"], batch["T_camera_pseudoCam"],
                                                               batch["T_world_pseudoCam"], batch["T_world_local"],
                                                               dtype=self.token_dtype)
            feat_hw = tuple(levels[layer].shape[-2:])
        else:
            feats = batch["all_features"]
            # encoding + `images_feat = features + encoding` + both einops rearranges, fused (parq_lightning.py:72-85)
            input_tokens = self.add_ray_pe.tokens(feats, batch["camera_feature"], batch["T_camera_pseudoCam"],
                                                  batch["T_world_pseudoCam"], batch["T_world_local"], dtype=self.token_dtype)
            feat_hw = tuple(feats.shape[-2:])
        outputs = self.box3d_decoder(input_tokens, batch["camera_feature"], batch["T_camera_pseudoCam"],
                                     batch["T_world_pseudoCam"], batch["T_world_local"], feat_hw=feat_hw)
        if "obbs_padded" in batch:
            self.box3d_decoder.settle_deferred()        # (InFlight) the loss reads the outputs on the host: a flagged forward is re-run first
            losses = self.box3d_decoder.loss(outputs, batch["obbs_padded"], batch["T_world_local"], batch["sym"])
        else:
            losses = {"total_loss": 0}
        return losses, outputs

    def validation_step(self, batch, batch_idx):
        """model/parq_lightning.py:102-112 without the TensorBoard logging: with ground truth in the batch the scene-level F1
        trackers are advanced by this snippet batch; with ``for_vis`` and ``box3d_decoder.draw_images`` the snippet's overlays
        are written to ``demo_vis/`` (:110-111)."""
        losses, outputs = self.forward(batch, batch_idx)
        if "obbs_padded" in batch:
            self.box3d_decoder.update_metrics(outputs, batch["obbs_padded"], batch["T_world_local"], batch["scene_name"])
        if self.for_vis and self.box3d_decoder.draw_images:
            self.vis_output(batch, outputs, output_name="demo_vis")
        return losses["total_loss"]

    def get_log_images(self, batch, outputs):
        """model/parq_lightning.py:256-293: tag -> uint8 NumPy ``(3, T*H, W)`` of ``box3d_decoder.log_images``' overlays (scene 0;
        ``{}`` while ``box3d_decoder.draw_images`` is off or the batch has no ``rgb_img``).  The bytes are the drawing kernel's
        own ``trunc(value * 255)`` output: one device-to-host copy per tag and no arithmetic on the host."""
        dec = self.box3d_decoder
        if not dec.draw_images or batch.get("rgb_img") is None:
            return {}
        images = dec._draw_log_images(outputs, batch.get("obbs_padded"), batch["T_world_pseudoCam"], batch["T_world_local"],
                                      batch["T_camera_pseudoCam"], batch["rgb_img"], batch["camera"], torch.uint8)
        return {tag: im.cpu().numpy() for tag, im in images.items()}

    @staticmethod
    def save_log_images(log_ims, directory, name):
        """Write every ``(3, H, W)`` uint8 array of ``log_ims`` to ``"{directory}/{name}_{tag}.png"`` (the directory is made)
        and return the paths.  Needs Pillow, imported here and nowhere else."""
        import os
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError("parq_amd.PARQ.save_log_images writes PNG files through Pillow (PIL), which is not installed; "
                               "get_log_images still returns the uint8 arrays") from e
        os.makedirs(directory, exist_ok=True)
        paths = []
        for tag, im in log_ims.items():
            path = os.path.join(directory, "%s_%s.png" % (name, tag))
            Image.fromarray(im.transpose(1, 2, 0)).save(path)
            paths.append(path)
        return paths

    def vis_output(self, batch, outputs, output_name="output"):
        """model/parq_lightning.py:295-304: the overlays of this snippet as ``{output_name}/{scene}_{snippet id}_{tag}.png``."""
        log_ims = self.get_log_images(batch, outputs)
        sid = batch["snippet_id"]
        sid = sid.reshape(-1)[0].item() if hasattr(sid, "reshape") else sid
        return self.save_log_images(log_ims, output_name, "%s_%s" % (batch["scene_name"][0], sid))

    def on_validation_epoch_start(self):
        self.box3d_decoder.reset_metrics()

    def validation_epoch_end(self, outs=None):
        """model/parq_lightning.py:118-142: {"0.25_f1", ...}; `eval.py` calls this directly and prints the result.  As in the
        reference the RETURNED dict is this rank's own; the scalars it logs with ``sync_dist=True`` (:133-140: mean over the
        ranks) are kept in ``self.synced_metrics`` and, under Lightning, logged the same way."""
        from .parallel import all_reduce_mean_scalars
        metrics = self.box3d_decoder.compute_metrics()
        self.synced_metrics = all_reduce_mean_scalars(metrics)
        if _Base is not nn.Module:                        # pragma: no cover - Lightning is absent on the target image
            for key, value in metrics.items():
                if isinstance(value, (int, float)):
                    self.log("val/metrics/{}".format(key), value, on_epoch=True, logger=True, sync_dist=True, rank_zero_only=False)
        return metrics

    def test_step(self, batch, batch_idx=0):
        return self.forward(batch, batch_idx)

    def training_step(self, batch, batch_idx):
        """model/parq_lightning.py:97-100.  In train mode the decoder forward is an autograd node whose backward is the HIP
        backward chain, and AddRayPE.tokens is an autograd node too: the decoder and the ray-PE
        encoder receive gradients, and d loss / d features is handed to whatever produced ``all_features`` (or the four
        ``fpn_features`` levels)."""
        losses, _ = self.forward(batch, batch_idx)
        return losses["total_loss"]

    def configure_optimizers(self):
        """AdamW with the reference's batch-size learning-rate rule and its warm-up + cosine-restart schedule, stepped per
        epoch (model/parq_lightning.py:150-199).  The reference's `torch.optim._multi_tensor.AdamW` no longer exists in
        torch 2 (`foreach=True` is the same implementation) and its 1-tuple return value is not inherited: this returns the
        Lightning dictionary itself, or the bare optimizer when the config carries no schedule section."""
        from .schedule import CosineAnnealingWarmupRestarts
        base = _get(self.cfg, "OPTIMIZER.LEARNING_RATE")
        lr, eff = base, None
        try:
            eff = (_get(self.cfg, "DATAMODULE.BATCH_SIZE") * _get(self.cfg, "TRAINER.NUM_NODES") * _get(self.cfg, "TRAINER.GPUS") *
                   _get(self.cfg, "TRAINER.ACCUMULATE_GRAD_BATCHES"))
            if _get(self.cfg, "OPTIMIZER.AUTOSCALE_LR"):
                lr = base * eff / 256.0
        except (KeyError, AttributeError):
            pass
        optimizer = torch.optim.AdamW([p for p in self.parameters() if p.requires_grad], lr=lr, foreach=True)
        try:
            warmup = _get(self.cfg, "OPTIMIZER.WARMUP_EPOCHS")
            mult = _get(self.cfg, "OPTIMIZER.CYCLE_MULT")
            restarts = _get(self.cfg, "OPTIMIZER.NUM_RESTARTS")
            epochs = _get(self.cfg, "TRAINER.MAX_EPOCHS")
        except (KeyError, AttributeError):
            return optimizer
        lr_min = base / 256.0 if (eff is not None and eff <= 256) else base
        cycle0 = math.ceil(epochs / sum(pow(mult, i) for i in range(restarts)))
        scheduler = CosineAnnealingWarmupRestarts(optimizer, cycle0, mult, lr, lr_min, warmup)
        return {"optimizer": optimizer, "lr_scheduler": {"scheduler": scheduler, "interval": "epoch"}}
