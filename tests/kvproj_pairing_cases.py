"""Cases of tests/test_gpu_kvproj_pairing.py, shared with tools/make_golden_kvproj_pairing.py, which recorded
tests/golden/kvproj_pairing.npz at the commit BEFORE the persistent K/V projection kernel's column slices were rebalanced and its
epilogue got one range decision per block.  Nothing here is an oracle: a case is one call of the project's own decoder, and the
recording is what that call returned then — outputs, range flag word, mirror words — compared bit for bit.

d = 256, 4 heads, Q = 32, 2 iterations, views of 8 x 8 = 64 keys (one row tile of kvproj_dma_kernel), range_check = "off" (one
forward, nothing re-run) unless the case says otherwise.  Key counts per scene:
  64       one tile: the two workgroups of a slot share a single tile
  192      an odd tile count
  576 x 2  B = 2: tiles of two scenes in one workgroup's sequence once the grid is smaller than the tile count
  2560     40 tiles; "x4" (B = 4) is 160 tiles — more than half the CUs of a 256-CU part, so workgroups walk several tiles and an
           epilogue's stores sit inside the k-loop's counted waits
Modes: split8 (stage cache), split8 with safe_heads 0b0101 (per-wave epilogues, wider regions), split (fp16 x 3 layout), fp16."""
import functools

import numpy as np
import torch

from parq_amd import synth

KEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d", "sem_cls_prob", "coord_pos")
GOLDEN = "kvproj_pairing.npz"
MODES = {"split8": ("split8", 0), "split8mix": ("split8", 0b0101), "split": ("split", 0), "fp16": ("fp16", 0)}
SIZES = {"n64": (1, 1), "n192": (1, 3), "n576x2": (2, 9), "n2560": (1, 40)}          # (B, views of 64 keys)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
WK = "parq_module.decoder.layers.0.multihead_attn.in_proj_weight"


def case_ids():
    ids = ["%s-%s-f32" % (s, m) for s in SIZES for m in MODES]
    ids += ["n192-%s-%s" % (m, t) for m in MODES for t in ("f16", "bf16")]
    ids += ["n2560x4-split8-f32", "n2560x4-split8mix-f32"]
    ids += ["window-split", "window-split8", "range-off", "range-lazy", "e4m3range-off"]
    return ids


@functools.lru_cache(maxsize=None)
def model(k_head1_scale=1.0, q_scale=1.0):
    cfg = synth.decoder_cfg(dim=256, queries=32, heads=4, ffn=768, layers=2)
    W = synth.make_decoder_weights(cfg, 7300, damped=True)
    if k_head1_scale != 1.0 or q_scale != 1.0:
        W = dict(W)
        w = W[WK].copy()
        w[256 + 64:256 + 128] *= np.float32(k_head1_scale)          # the K rows of head 1
        w[:256] *= np.float32(q_scale)                              # the query rows: rows that spread over all keys (fixture g21's recipe)
        W[WK] = w
    return cfg, W


@functools.lru_cache(maxsize=None)
def scene(seed, B, V, hw=8):
    return synth.make_scene(seed, B, V, hw, hw, 256)


def range_scene(row_scale):
    """N = 192 with token row 70 of scene 0 scaled: every element of the row stays far inside the fp16 range."""
    sc = dict(scene(7340, 1, 3))
    tok = sc["tokens"].copy()
    tok.reshape(1, 192, 256)[0, 70] *= np.float32(row_scale)
    sc["tokens"] = tok
    return sc


def k_of_row(W, sc, row):
    """float64 K of one token row, per head: what the range cases are built on (checked on the CPU by the recording tool)."""
    w = W[WK].astype(np.float64)[256:512]
    b = W[WK.replace("weight", "bias")].astype(np.float64)[256:512]
    return (sc["tokens"].reshape(-1, 256)[row].astype(np.float64) @ w.T + b).reshape(4, 64)


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dtype)


def _args(sc, dtype):
    return (_dev(sc["tokens"], dtype), _dev(sc["camera"]), _dev(sc["T_camera_pseudoCam"]), _dev(sc["T_world_pseudoCam"]),
            _dev(sc["T_world_local"]))


def _decoder(mode, safe, range_check, k_head1_scale=1.0, q_scale=1.0):
    from gpu_util import make_decoder
    cfg, W = model(k_head1_scale, q_scale)
    dec = make_decoder(cfg, W).eval()
    dec.attention_mode, dec.safe_heads, dec.range_check = mode, safe, range_check
    return dec


def _record(outs, flag, mirror, dec):
    torch.cuda.synchronize()
    rec = {"it%d.%s" % (i, k): o[k].detach().cpu().numpy().copy() for i, o in enumerate(outs) for k in KEYS}
    rec["flag"] = flag.cpu().numpy().copy()
    rec["mirror"] = np.asarray(mirror).copy()
    rec["state"] = np.array([dec.safe_heads, {"split8": 4, "split": 1, "fp16": 2, "fp32": 0}[dec.attention_mode]], np.int64)
    return rec


def run(case_id):
    """One case on cuda:0 -> {name: ndarray}: the six outputs of both iterations, the workspace's range flag word, the 16 mirror
    words as the host sees them right after the forward, (safe_heads, attention mode) after it."""
    parts = case_id.split("-")
    with torch.no_grad():
        if parts[0] == "window":
            # fill, forward, replace view 1, forward: the second forward projects the rows of view 1 only.  "split": 3 views of 64
            # keys, rows [64, 128).  "split8": a row of that mode has to rest on 256 keys' worth of probability or the forward raises
            # the too-peaked bit, after which a window projects everything — so 4 views of 16 x 16 with the query rows x 0.1
            V, hw, qs = (3, 8, 1.0) if parts[1] == "split" else (4, 16, 0.1)
            dec = _decoder(parts[1], 0, "off", q_scale=qs)
            a, b = scene(7320, 1, V, hw), scene(7321, 1, V, hw)
            t = _args(a, torch.float32)
            win = dec.view_window(1, V, hw, hw, t[4])
            win.put(list(range(V)), t[0], t[1], t[2], t[3])
            win.forward()
            u = _args(b, torch.float32)
            win.put(1, u[0].view(1, V, hw * hw, 256)[:, 1], u[1][:, [1]], u[2][:, [1]], u[3][:, [1]])
            outs = win.forward()
            torch.cuda.synchronize()
            assert win.last_projected_views == [1] and win.last_projected_rows == hw * hw, (win.last_projected_views, win.last_projected_rows)
            rec = _record(outs, dec._flag_view(win._entry.ws, 1, V, hw, hw), dec._mirror_np[:dec._MIRROR_SLOTS], dec)
            win.close()
            return rec
        if parts[0] in ("range", "e4m3range"):
            # range: token row 70 x 1000 and the K rows of head 1 x 100 — K of that row leaves the fp16 range in head 1 only
            # e4m3range: the row x 1000 alone — K beyond the e4m3 range (448) of the stage cache's 8-bit planes, inside fp16's: no flag
            dec = _decoder("split8", 0, parts[1], 100.0 if parts[0] == "range" else 1.0)
            sc = range_scene(1000.0)
            if parts[1] == "lazy":
                dec._ensure_packed(torch.device("cuda", torch.cuda.current_device()))
                dec._peaky_checked = True          # past the module's first forward, which every policy but "off" checks and re-runs
            outs = dec(*_args(sc, torch.float32))
            torch.cuda.synchronize()
            (B, V, h, w, _, _), ws = dec._last_ws()
            return _record(outs, dec._flag_view(ws, B, V, h, w), dec._mirror_np[:dec._MIRROR_SLOTS], dec)
        size, mode, tt = parts
        B, V = (4, 40) if size == "n2560x4" else SIZES[size]
        dec = _decoder(MODES[mode][0], MODES[mode][1], "off")
        outs = dec(*_args(scene(7310 + V, B, V), DTYPES[tt]))
        torch.cuda.synchronize()
        (B, V, h, w, _, _), ws = dec._last_ws()
        return _record(outs, dec._flag_view(ws, B, V, h, w), dec._mirror_np[:dec._MIRROR_SLOTS], dec)
