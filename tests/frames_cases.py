"""Cases, inputs and the NumPy statement of the frame preparation (parq_amd/frames.py, include/parq_hip.h parq_frames_resize).

The resize rule is Pillow's ``Image.resize(size, Image.BILINEAR)`` on 8-bit RGB restated in integers (``axis_plan`` +
``resize_statement``): tests/golden/g24_frames.npz holds what the reference's own transforms (Pillow underneath) gave for every
case (tools/make_golden_frames.py), the statement is pinned to those bytes, and the kernel to both.  Inputs are generated — an
integer hash of (n, y, x, c), no library RNG — so that only results are stored.
"""
import json
import math
import os

import numpy as np

G24 = "g24_frames"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", G24 + ".npz")
TILE_W, TILE_H = 32, 8                 # the kernel's output tile (csrc/frames.hip kTileW, kTileH)

# in = (W, H) of the frames, out = (w, h); pad = (left, top, right, bottom), "scannet" or None; fill: "hash", 255 or 0 per frame
RESIZE_CASES = [
    dict(name="odd_53x37", n=3, inp=(53, 37), out=(16, 12), pad=None),                       # 159-byte rows, 3.3x / 3.1x, 9 taps
    dict(name="pad_top_bottom", n=1, inp=(53, 33), out=(16, 12), pad=(0, 2, 0, 2)),
    dict(name="pad_left_right", n=2, inp=(50, 36), out=(16, 12), pad=(2, 1, 1, 0)),
    dict(name="upscale", n=1, inp=(13, 10), out=(20, 17), pad=None),
    dict(name="identity_x", n=1, inp=(16, 31), out=(16, 12), pad=None),
    dict(name="identity_y", n=1, inp=(31, 12), out=(16, 12), pad=None),
    dict(name="white_black", n=2, inp=(53, 37), out=(16, 12), pad=None, fill=(255, 0)),
    dict(name="tiles_83x45", n=2, inp=(211, 157), out=(83, 45), pad=None),                   # 3 x 6 tiles of 32 x 8, ragged both ways
    dict(name="down_7p8", n=1, inp=(250, 63), out=(32, 8), pad=None),                        # 17 taps; the tile's 63 rows are staged in 2 chunks
    dict(name="scannet", n=1, inp=(1296, 968), out=(320, 240), pad="scannet"),               # the reference's own shape
]
# B scenes of T views; the frames (for FramePrep end to end) are those of the resize case `frames`, (B*T) of them
POSE_CASES = [
    dict(name="poses_t3", B=1, T=3, inp=(53, 37), out=(16, 12), pad=None),
    dict(name="poses_t9", B=1, T=9, inp=(1296, 968), out=(320, 240), pad="scannet"),
    dict(name="poses_b2", B=2, T=3, inp=(53, 37), out=(16, 12), pad=None, frames=True),
]


def pad4(pad, inp):
    if pad == "scannet":
        return (0, 2, 0, 2) if tuple(inp) == (1296, 968) else (0, 0, 0, 0)
    return (0, 0, 0, 0) if pad is None else tuple(pad)


def _mix(v):
    v = (v ^ (v >> 15)) & 0xFFFFFFFF
    v = (v * 0x2C1B3C6D) & 0xFFFFFFFF
    v = (v ^ (v >> 12)) & 0xFFFFFFFF
    v = (v * 0x297A2D39) & 0xFFFFFFFF
    return (v ^ (v >> 15)) & 0xFFFFFFFF


def _hash(n, y, x, c, seed):
    v = (n * 0x3A8F05C5 + y * 0x1B873593 + x * 0x0CC9E2D5 + c * 0x06546B64 + seed) & 0xFFFFFFFF
    return _mix(v)


def make_frames(n, W, H, seed=0, fill=None):
    """(n, H, W, 3) uint8: blocks of 4 x 4 pixels of a hashed level plus hashed 5-bit detail, all in int64 masked to 8 bits;
    `fill`: one constant per frame instead."""
    if fill is not None:
        return np.stack([np.full((H, W, 3), f, np.uint8) for f in fill])
    nn, yy, xx, cc = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64),
                                 np.arange(3, dtype=np.int64), indexing="ij")
    v = _hash(nn, yy // 4, xx // 4, cc, seed) + (_hash(nn, yy, xx, cc, seed + 1) & 31)
    return (v & 255).astype(np.uint8)


def case_frames(c):
    if "B" in c:
        return make_frames(c["B"] * c["T"], c["inp"][0], c["inp"][1], seed=len(c["name"]))
    return make_frames(c["n"], c["inp"][0], c["inp"][1], seed=len(c["name"]), fill=c.get("fill"))


# ---------------------------------------------------------------------------------------------------------------- the statement
def axis_plan(inp, out):
    """ksize, xmin (out,), n (out,), k (out, ksize) int32: the coefficient plan of one axis, in float64, operation by operation."""
    scale = inp / out
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    xmin, n, k = np.zeros(out, np.int32), np.zeros(out, np.int32), np.zeros((out, ksize), np.int32)
    for xx in range(out):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), inp) - lo
        w = [max(0.0, 1.0 - abs((x + lo - center + 0.5) * ss)) for x in range(cnt)]
        ww = 0.0
        for v in w:
            ww += v
        xmin[xx], n[xx] = lo, cnt
        for x in range(cnt):
            k[xx, x] = int(0.5 + (w[x] / ww) * 4194304)
    return ksize, xmin, n, k


def plan_ints(inp, out):
    """The plan as parq_frame_plan lays it out: [ksize, (xmin, n, k[0..ksize)) per output index] int32."""
    ksize, xmin, n, k = axis_plan(inp, out)
    return np.concatenate([[ksize], np.concatenate([xmin[:, None], n[:, None], k], axis=1).reshape(-1)]).astype(np.int32)


def _pass(a, axis, inp, out):
    """One pass along `axis` of the int64 array a (values 0..255): rounded to 8 bits, clipped."""
    _, xmin, n, k = axis_plan(inp, out)
    a = np.moveaxis(a, axis, 0)
    res = np.zeros((out,) + a.shape[1:], np.int64)
    for xx in range(out):
        seg = a[xmin[xx]:xmin[xx] + n[xx]]
        kk = k[xx, :n[xx]].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
        res[xx] = np.clip((2097152 + (seg * kk).sum(0)) >> 22, 0, 255)
    return np.moveaxis(res, 0, axis)


def resize_statement(frames, pad, out):
    """(N, 3, h, w) uint8 from (N, H, W, 3) uint8 frames: zero border, horizontal pass rounded to 8 bits, vertical pass."""
    N, H, W, _ = frames.shape
    l, t, r, b = pad
    w, h = out
    padded = np.zeros((N, H + t + b, W + l + r, 3), np.int64)
    padded[:, t:t + H, l:l + W] = frames
    tmp = _pass(padded, 2, W + l + r, w)
    res = _pass(tmp, 1, H + t + b, h)
    return np.ascontiguousarray(res.transpose(0, 3, 1, 2)).astype(np.uint8)


def as_float(bytes_):
    """What ToTensor + Normalize make of the bytes: one correctly rounded float32 division."""
    return bytes_.astype(np.float32) / np.float32(255)


# ---------------------------------------------------------------------------------------------------------------- poses, intrinsics
def _rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    return np.array({"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
                     "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis], np.float64)


def case_poses(c):
    """intrinsics (B, T, 3, 3) float64 of the raw frames (every view its own) and T_world_camera (B, T, 4, 4) float32: cameras on an
    arc, pitched and rolled, up to 8 m from the origin; no view looks along the world's z."""
    B, T = c["B"], c["T"]
    W, H = c["inp"]
    K = np.zeros((B, T, 3, 3), np.float64)
    M = np.zeros((B, T, 4, 4), np.float32)
    for b in range(B):
        for t in range(T):
            i = b * T + t
            f = 0.9 * W + 0.37 * i
            K[b, t] = [[f, 0, (W - 1) / 2 + 0.25 * i], [0, f * 1.003, (H - 1) / 2 - 0.125 * i], [0, 0, 1]]
            R = _rot("z", 0.7 * i - 1.3 + b) @ _rot("x", -(1.25 + 0.09 * ((i * 5) % 7))) @ _rot("z", 0.11 * ((i * 3) % 5) - 0.2)
            M[b, t, :3, :3] = R
            M[b, t, :3, 3] = [8.0 * math.cos(1.1 * i + b), -8.0 * math.sin(0.7 * i), 1.0 + 0.15 * i]
            M[b, t, 3, 3] = 1
    return K, M


def pose_bound(T_world_camera):
    """Per-entry bound on float32 pose differences: 16 roundings of quantities no larger than max(1, max |t|)."""
    return 16 * 2.0 ** -24 * max(1.0, float(np.abs(np.asarray(T_world_camera)[..., :3, 3]).max()))


def load_golden():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta
