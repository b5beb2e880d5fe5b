"""Write tests/golden/g24_frames.npz: the reference's own frame preparation on the cases of tests/frames_cases.py.

Development container only (it imports the reference tree through oracle.reference_loader and needs Pillow; run from the
repository root: ``python tools/make_golden_frames.py``).  Per resize case the frames (a custom border added with
``ImageOps.expand``, as ``pad_scannet`` adds its own) go through the reference's ``ResizeImage`` + ``ToTensor`` + ``Normalize``
(datasets/transforms.py); stored are the resized BYTES ``(N, 3, h, w)``, after checking that the normalised float32 images are
exactly ``bytes / 255``.  Per pose case every scene goes through ``ResizeImage`` / ``ToTensor`` / ``Normalize`` /
``Convert2Objects`` / ``GravityAligned`` / ``SnippetLocal``; stored are the float32 camera rows, ``T_world_pseudoCam``,
``T_camera_pseudoCam``, ``T_world_local`` and, where the case carries frames, their resized bytes.  A ``meta`` JSON lists the cases.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frames_cases as FC  # noqa: E402
from oracle import reference_loader  # noqa: E402


def chain(T, size):
    from datasets import transforms as RT
    return RT.Compose([RT.ResizeImage(size), RT.ToTensor(), RT.Normalize(), RT.Convert2Objects(T),
                       RT.GravityAligned(dataset_type="SCANNET"), RT.SnippetLocal()])


def images(frames, border):
    from PIL import Image, ImageOps
    ims = [Image.fromarray(f, "RGB") for f in frames]
    return [ImageOps.expand(im, border=border) for im in ims] if border else ims


def run_scene(frames, K, M, c):
    """One scene (T views) through the reference's chain.  A border the reference would not add itself is added to the images and to
    the principal point here, as pad_scannet does for its own."""
    T = len(frames)
    pad = FC.pad4(c["pad"], c["inp"])
    own = tuple(c["inp"]) == (1296, 968) and pad == (0, 2, 0, 2)
    K = [k.copy() for k in K]
    if not own:
        for k in K:
            k[0, 2] += pad[0]
            k[1, 2] += pad[1]
    data = {"rgb_img": images(frames, None if own or not any(pad) else pad), "intrinsics": K, "T_world_camera": M.copy(), "bboxes": None}
    out = chain(T, tuple(c["out"]))(data)
    bytes_ = torch.round(out["rgb_img"] * 255).to(torch.uint8).numpy()
    assert np.array_equal(out["rgb_img"].numpy().view(np.uint32), FC.as_float(bytes_).view(np.uint32))
    return bytes_, out


def main():
    reference_loader.load()
    arrays = {}
    for c in FC.RESIZE_CASES:
        frames = FC.case_frames(c)
        W, H = c["inp"]
        K = [np.array([[W, 0, W / 2], [0, W, H / 2], [0, 0, 1]], np.float64) for _ in frames]
        M = np.tile(np.eye(4, dtype=np.float32), (len(frames), 1, 1))
        M[:, 0, 2], M[:, 2, 2], M[:, 2, 0], M[:, 0, 0] = 1, 0, -1, 0          # a forward axis that is not the world's up
        bytes_, _ = run_scene(frames, K, M, c)
        assert bytes_.shape == (c["n"], 3, c["out"][1], c["out"][0])
        arrays[c["name"] + "/bytes"] = bytes_
        print("%s: %s -> %s, mean byte %.2f" % (c["name"], frames.shape, bytes_.shape, bytes_.mean()))
    for c in FC.POSE_CASES:
        K, M = FC.case_poses(c)
        B, T = c["B"], c["T"]
        frames = FC.case_frames(c) if c.get("frames") else np.zeros((B * T, c["inp"][1], c["inp"][0], 3), np.uint8)
        frames = frames.reshape((B, T) + frames.shape[1:])
        per = [run_scene(frames[b], list(K[b]), M[b], c) for b in range(B)]
        p = c["name"] + "/"
        arrays[p + "camera"] = np.stack([o["camera"]._data.numpy() for _, o in per]).astype(np.float32)
        for key in ("T_world_pseudoCam", "T_camera_pseudoCam", "T_world_local"):
            arrays[p + key] = np.stack([o[key]._data.numpy() for _, o in per]).astype(np.float32)
        if c.get("frames"):
            arrays[p + "bytes"] = np.stack([b for b, _ in per])
        print("%s: camera %s, T_world_local %s" % (c["name"], arrays[p + "camera"].shape, arrays[p + "T_world_local"].shape))
    meta = {"resize": FC.RESIZE_CASES, "poses": FC.POSE_CASES}
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(FC.GOLDEN, **arrays)
    print("wrote %s (%d arrays, %d bytes)" % (FC.GOLDEN, len(arrays), os.path.getsize(FC.GOLDEN)))


if __name__ == "__main__":
    main()
