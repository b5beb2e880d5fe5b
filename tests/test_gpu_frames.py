"""GPU tier of the frame preparation (parq_amd.resize_frames / FramePrep / FeatureViewWindow.put_frames; include/parq_hip.h
parq_frames_resize, csrc/frames.hip).  The resize is held to "every byte equal": to the bytes the reference's own transforms gave
(tests/golden/g24_frames.npz) and to the NumPy statement of the rule (tests/frames_cases.py).  The cases are the smallest that
reach what they name: rows of 159 bytes, borders on each side, an upscale, an identity axis, constant frames, more than one
32 x 8 tile in both directions with ragged edges, a tile whose input rows are staged in two chunks, the reference's own shape."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from parq_amd import Camera, Pose, _lib, synth
from parq_amd import frames as F

import frames_cases as FC

pytestmark = pytest.mark.gpu

Z, META = FC.load_golden()
RESIZE_IDS = [c["name"] for c in FC.RESIZE_CASES]
KEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d", "sem_cls_prob", "coord_pos")
_statement = {}


def statement(c):
    if c["name"] not in _statement:
        res = FC.resize_statement(FC.case_frames(c), FC.pad4(c["pad"], c["inp"]), tuple(c["out"]))
        res.setflags(write=False)
        _statement[c["name"]] = res
    return _statement[c["name"]]


def _pad(c):
    return c["pad"] if c["pad"] is None or isinstance(c["pad"], str) else tuple(c["pad"])


@pytest.mark.parametrize("c", FC.RESIZE_CASES, ids=RESIZE_IDS)
def test_bytes_equal_the_fixture_and_the_statement(c):
    frames = torch.from_numpy(FC.case_frames(c)).cuda()
    got = F.resize_frames(frames, tuple(c["out"]), _pad(c), dtype=torch.uint8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (c["n"], 3, c["out"][1], c["out"][0])
    got = got.cpu().numpy()
    diff = int((got != Z[c["name"] + "/bytes"]).sum())
    print("%s: %d of %d bytes differ from the fixture" % (c["name"], diff, got.size))
    assert diff == 0
    assert np.array_equal(got, statement(c))


@pytest.mark.parametrize("c", FC.RESIZE_CASES, ids=RESIZE_IDS)
def test_float32_is_bit_equal_to_bytes_over_255(c):
    frames = torch.from_numpy(FC.case_frames(c)).cuda()
    got = F.resize_frames(frames, tuple(c["out"]), _pad(c))
    assert got.dtype == torch.float32
    want = FC.as_float(Z[c["name"] + "/bytes"])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_all_256_values_divide_as_numpy_does():
    frames = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous().cuda()
    got = F.resize_frames(frames, (16, 16), None).cpu().numpy()                  # both axes the identity plan
    want = FC.as_float(np.arange(256, dtype=np.uint8).reshape(1, 1, 16, 16).repeat(3, 1))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_a_buffer_at_any_byte_alignment(offset):
    """Frames that start 1, 2, 3 bytes past a dword boundary and end anywhere: the first and the last dword of the buffer are not wholly
    inside it.  The bytes around the frames are 0xFF: any of them read as a pixel shows up in the output."""
    c = FC.RESIZE_CASES[0]
    fr = FC.case_frames(c)
    buf = torch.full((offset + fr.size + 8,), 255, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + fr.size].view(fr.shape)
    view.copy_(torch.from_numpy(fr))
    assert view.data_ptr() % 4 == offset and view.is_contiguous()
    got = F.resize_frames(view, tuple(c["out"]), None, dtype=torch.uint8).cpu().numpy()
    assert np.array_equal(got, statement(c))


def test_leading_dimensions_out_and_a_side_stream():
    c = FC.POSE_CASES[2]
    fr = torch.from_numpy(FC.case_frames(c).reshape(2, 3, 37, 53, 3)).cuda()
    want = Z[c["name"] + "/bytes"]
    out = torch.full((2, 3, 3, 12, 16), 7, dtype=torch.uint8, device="cuda")
    assert F.resize_frames(fr, (16, 12), "scannet", dtype=torch.uint8, out=out) is out
    assert np.array_equal(out.cpu().numpy(), want)
    one = F.resize_frames(fr[1, 2], (16, 12), dtype=torch.uint8)                   # a single (H, W, 3) frame
    assert tuple(one.shape) == (3, 12, 16) and np.array_equal(one.cpu().numpy(), want[1, 2])
    outf = torch.full((2, 3, 3, 12, 16), -1.0, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert F.resize_frames(fr, (16, 12), out=outf) is outf
    side.synchronize()
    assert np.array_equal(outf.cpu().numpy().view(np.uint32), FC.as_float(want).view(np.uint32))


def _pose_inputs(c):
    K, M = FC.case_poses(c)
    fr = FC.case_frames(c).reshape((c["B"], c["T"], c["inp"][1], c["inp"][0], 3))
    return torch.from_numpy(fr).cuda(), torch.from_numpy(K), torch.from_numpy(M)


def test_frame_prep_end_to_end_on_two_scenes():
    c = FC.POSE_CASES[2]
    fr, K, M = _pose_inputs(c)
    batch = F.FramePrep(size=tuple(c["out"]))(fr, K, M)
    assert sorted(batch) == ["T_camera_pseudoCam", "T_world_camera", "T_world_local", "T_world_pseudoCam", "camera", "rgb_img"]
    p = c["name"] + "/"
    rgb = batch["rgb_img"]
    assert rgb.is_cuda and rgb.dtype == torch.float32 and tuple(rgb.shape) == (2, 3, 3, 12, 16)
    assert np.array_equal(rgb.cpu().numpy().view(np.uint32), FC.as_float(Z[p + "bytes"]).view(np.uint32))
    assert isinstance(batch["camera"], Camera) and all(isinstance(batch[k], Pose) for k in batch if k.startswith("T_"))
    bound = FC.pose_bound(M.numpy())
    for key in ("camera", "T_world_pseudoCam", "T_camera_pseudoCam", "T_world_local"):
        got, want = batch[key]._data, Z[p + key]
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max())
        print("%s: max |a - b| = %.3e, bound %.3e" % (key, err, bound))
        assert err <= bound
    assert np.array_equal(batch["camera"]._data.cpu().numpy().view(np.uint32), Z[p + "camera"].view(np.uint32))      # float64 on both sides
    assert torch.equal(batch["T_world_camera"]._data.cpu(), Pose.from_4x4mat(M)._data)
    own = F.FramePrep(size=tuple(c["out"]), first_view_intrinsics=False)(fr, K, M)["camera"]._data.cpu()
    assert torch.equal(own[:, 0], batch["camera"]._data.cpu()[:, 0]) and not torch.equal(own[:, 1], own[:, 0])


class _PoolBackbone(torch.nn.Module):
    """A stand-in 2-D backbone: 2 x 2 average pooling of ``rgb_img``, the three channels spread over C with fixed gains."""

    def __init__(self, C_):
        super().__init__()
        self.C = C_

    def forward(self, batch):
        img = batch["rgb_img"]
        B, T = img.shape[:2]
        pooled = torch.nn.functional.avg_pool2d(img.flatten(0, 1), 2).unflatten(0, (B, T))
        gain = (0.5 + torch.arange(self.C, device=img.device, dtype=torch.float32) / self.C).view(1, 1, -1, 1, 1)
        batch["all_features"] = (pooled[:, :, torch.arange(self.C, device=img.device) % 3] * gain).contiguous()
        batch["camera_feature"] = batch["camera"].scale(0.5)
        return batch


def _module(backbone):
    from types import SimpleNamespace as NS
    from parq_amd import PARQ
    Cd = 256
    dcfg = synth.decoder_cfg(dim=Cd, queries=32, heads=4, ffn=768, layers=2)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg))
    model = PARQ(cfg, backbone2d=backbone).eval()
    W, Wp = synth.make_decoder_weights(dcfg, 6311, damped=True), synth.make_ray_pe_weights(Cd, 6312)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("box3d_decoder."):
            sd[k] = torch.from_numpy(W[k[len("box3d_decoder."):].replace("parq_module.decoder.mlp_heads.", "mlp_heads.")]).reshape(sd[k].shape)
        else:
            sd[k] = torch.from_numpy(Wp[k[len("add_ray_pe."):]])
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    model.box3d_decoder.attention_mode = "split"
    return model


def _forward(fn, *a):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            outs = fn(*a)
    outs = [{k: o[k].clone() for k in KEYS} for o in outs]
    torch.cuda.synchronize()
    return outs


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in KEYS)


def test_put_frames_equals_put_features_of_the_prepared_views():
    c = FC.POSE_CASES[2]
    fr, K, M = _pose_inputs(c)
    B, V, (h, w) = c["B"], c["T"], (6, 8)
    backbone = _PoolBackbone(256)
    model = _module(backbone)
    prep = F.FramePrep(size=tuple(c["out"]), first_view_intrinsics=False)
    whole = prep(fr, K, M)
    T_wl = whole["T_world_local"]
    puts = ([0], [1, 2])

    win = model.view_window(B, V, h, w, T_wl)
    for sl in puts:
        b = backbone(prep(fr[:, sl].contiguous(), K[:, sl], M[:, sl]))
        win.put_features(sl if len(sl) > 1 else sl[0], b["all_features"], b["camera_feature"], b["T_camera_pseudoCam"], b["T_world_pseudoCam"])
    torch.cuda.synchronize()
    want = {k: getattr(win, k).clone() for k in ("tokens", "camera", "T_camera_pseudoCam", "T_world_pseudoCam", "T_world_local")}
    want_out = _forward(win.forward)
    win.close()

    win = model.view_window(B, V, h, w, T_wl)
    win.frame_prep = prep
    for sl in puts:
        win.put_frames(sl if len(sl) > 1 else sl[0], fr[:, sl].contiguous(), K[:, sl], M[:, sl])
    torch.cuda.synchronize()
    for k, v in want.items():
        assert torch.equal(getattr(win, k), v), k
    assert torch.equal(win.T_world_local, T_wl._data)                               # what the window was given, not the put views' own
    assert _same(_forward(win.forward), want_out)
    assert _same(_forward(lambda: model(whole, 0)[1]), want_out)                    # and the module's forward on the whole prepared batch
    win.close()

    assert win.frame_prep is prep
    bare = _module(None)
    win = bare.view_window(B, V, h, w, T_wl)
    with pytest.raises(ValueError, match="backbone2d"):
        win.put_frames(0, fr[:, [0]].contiguous(), K[:, [0]], M[:, [0]])
    with pytest.raises(ValueError):
        model.view_window(B, V, h, w, T_wl).put_frames([0, 1], fr[:, [0]].contiguous(), K[:, [0]], M[:, [0]])
    win.close()


def test_the_c_abi_refuses_each_argument_class_and_launches_nothing():
    lib = _lib.load()
    c = FC.RESIZE_CASES[0]
    fr = torch.from_numpy(FC.case_frames(c)).cuda()
    (W, H), (w, h) = c["inp"], c["out"]
    px, py = (torch.from_numpy(F.frame_plan(a, b)).cuda() for a, b in ((W, w), (H, h)))
    out = torch.full((3, 3, h, w), 171, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    good = dict(frames=p(fr), N=3, H_in=H, W_in=W, pl=0, pt=0, pr=0, pb=0, plan_x=p(px), plan_y=p(py), H_out=h, W_out=w, out=p(out), u8=1)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.parq_frames_resize(*a.values(), _lib.stream_ptr())

    bad = [dict(frames=None), dict(plan_x=None), dict(plan_y=None), dict(out=None), dict(N=0), dict(N=-1), dict(N=65536), dict(H_in=0),
           dict(W_in=0), dict(H_out=0), dict(W_out=-2), dict(pl=-1), dict(pt=-1), dict(pr=-1), dict(pb=-1), dict(H_in=8193),
           dict(W_in=8193), dict(H_out=8193), dict(W_out=8193), dict(pr=8192 - W + 1), dict(pb=8192), dict(u8=2), dict(u8=-1),
           dict(W_out=6), dict(H_out=4), dict(pt=h * 8 - H + 1)]
    for kw in bad:
        assert call(**kw) == 1, kw                                                   # PARQ_ERR_ARG
        assert b"parq_frames_resize" in lib.parq_last_error()
    torch.cuda.synchronize()
    assert bool((out == 171).all()), "a refused call launched something"
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), statement(c))
