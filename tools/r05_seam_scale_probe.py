"""GPU box: the feature / weight scale sweep of tests/test_gpu_range.py with the norm1 seam as two launches (the default) and as one
(PARQDecoder.fuse_seams = True, i.e. parq_set_seam_fusion(h, 1)).  Prints the worst teacher-forced error against float64 per mode
and setting (profiles/r05_seam_scale_probe.txt)."""
import os
import sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import torch
torch.set_grad_enabled(False)
import test_gpu_range as T

_make = T.make_decoder
for fuse in (False, True):
    def make_decoder(cfg, W, _fuse=fuse):
        dec = _make(cfg, W)
        dec.fuse_seams = _fuse
        return dec
    T.make_decoder = make_decoder          # _decoder_errors builds its decoder through the module's name
    for fs in (1e-3, 1.0, 1e2):
        for wsc in (0.1, 1.0, 10.0):
            e = {m: T._decoder_errors(fs, wsc, m)[0] for m in ("split", "fp32")}
            print("fuse_seams=%d features x%g in-proj x%g: split %.2e fp32 %.2e" % (fuse, fs, wsc, e["split"], e["fp32"]), flush=True)
