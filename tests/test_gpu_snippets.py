"""GPU tier of the snippet targets (parq_amd.SnippetTargets; include/parq_hip.h parq_snippet_targets, csrc/snippets.hip).  The two
kernels are held to the NumPy statement of the rule (tests/snippet_cases.py) bit for bit — int32 counts per frame and per snippet,
float32 ratio bits, levels, valid flags, num_valid, obbs_padded, sym — and to what the reference's own functions gave
(tests/golden/g25_snippets.npz) under the terms of the CPU tier: counts, levels and rows exactly, ratios at 1e-4.  The cases are the
smallest that reach what they name (tests/snippet_cases.py CASES)."""
import ctypes as C

import numpy as np
import pytest
import torch

from parq_amd import Obb3D, Pose, SnippetTargets, _lib, synth
from parq_amd import frames as F
from parq_amd.wrappers import raw

import snippet_cases as SC
from gpu_util import make_decoder

pytestmark = pytest.mark.gpu

Z, META = SC.load_golden()
IDS = [c["name"] for c in SC.CASES]
KEYS = ("frame_points", "frame_truncation", "points_inside", "truncation", "difficulty", "valid", "obbs_padded", "sym", "num_valid")
_statement = {}


def statement(c, **kw):
    key = (c["name"], tuple(sorted(kw.items())))
    if key not in _statement:
        res = SC.case_statement(c, **kw)
        for v in res.values():
            v.setflags(write=False)
        _statement[key] = res
    return _statement[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_equals_statement(got, want, what):
    for key in KEYS:
        g, w = got[key], want[key]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, key, g.shape, g.dtype, w.shape, w.dtype)
        bad = int((_bits(g) != _bits(w)).sum())
        if bad:
            print("%s %s: %d of %d differ\n got  %s\n want %s" % (what, key, bad, g.size, g.ravel()[:24], w.ravel()[:24]))
        assert bad == 0, (what, key)


def inputs(c):
    d = SC.make_case(c)
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items() if isinstance(v, np.ndarray) and "intrinsics" not in k}
    return d, [t["depth"], torch.from_numpy(d["depth_intrinsics"]), torch.from_numpy(d["color_intrinsics"]), d["color_size"],
               t["T_world_camera"], t["obbs"], t["sym"]], t.get("corners_world")


def from_module(res):
    out = {k: res[k].cpu().numpy() for k in ("points_inside", "truncation", "difficulty", "valid", "sym", "num_valid")}
    out["frame_points"], out["frame_truncation"] = res["frame_points_inside"].cpu().numpy(), res["frame_truncation"].cpu().numpy()
    out["obbs_padded"] = res["obbs_padded"]._data.cpu().numpy()
    return out


def run_module(c, **kw):
    d, args, corners = inputs(c)
    res = SnippetTargets(**kw)(*args, corners_world=corners, details=True)
    assert isinstance(res["obbs_padded"], Obb3D) and res["num_valid"].dtype == torch.int32 and res["valid"].dtype == torch.bool
    assert all(raw(v).is_cuda for v in res.values())
    return from_module(res)


def abi_call(d, levels=SC.DEFAULT_LEVELS, max_level=3, max_box=100, depth_scale=1000.0, stream=None, fill=None, **over):
    """parq_snippet_targets on the case's inputs; returns (rc, outputs as NumPy).  `over` replaces named arguments (tests of refusals);
    `fill`: the outputs are preset to this byte to show that a refused call wrote nothing."""
    lib = _lib.load()
    depth = torch.from_numpy(d["depth"]).cuda()
    B, T, Hd, Wd = depth.shape
    N, S = d["obbs"].shape[1], d["sym"].shape[1]
    Ki = torch.from_numpy(np.stack([np.linalg.inv(K) for K in d["depth_intrinsics"]])).cuda()
    Kc = torch.from_numpy(d["color_intrinsics"]).cuda()
    M = torch.from_numpy(np.concatenate([d["T_world_camera"][..., :3, :3].reshape(B, T, 9), d["T_world_camera"][..., :3, 3]], -1)).cuda()
    rows, sym = torch.from_numpy(d["obbs"]).cuda(), torch.from_numpy(d["sym"]).cuda()
    corners = torch.from_numpy(d["corners_world"]).cuda() if d["corners_world"] is not None else None
    need = lib.parq_snippet_targets_workspace(B, T, Hd, Wd, N)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    ws[need:] = 0xA5                                                                # the call must not write behind its workspace
    mk = lambda shape, dt: torch.full(shape, fill, dtype=dt, device="cuda") if fill is not None else torch.empty(shape, dtype=dt, device="cuda")
    out = dict(obbs_padded=mk((B, max_box, 19), torch.float32), sym_out=mk((B, S), sym.dtype), num_valid=mk((B,), torch.int32),
               frame_points=mk((B, T, N), torch.int32), frame_truncation=mk((B, T, N), torch.float32), points_inside=mk((B, N), torch.int32),
               truncation=mk((B, N), torch.float32), difficulty=mk((B, N), torch.int32), valid=mk((B, N), torch.int32))
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    n = len(levels)
    a = dict(depth=p(depth), B=B, T=T, Hd=Hd, Wd=Wd, kinv=p(Ki), kc=p(Kc), color_h=d["color_size"][0], color_w=d["color_size"][1], poses=p(M),
             obbs=p(rows), corners=p(corners), sym=p(sym), sym_is_int=int(sym.dtype == torch.int32), S=S, N=N, max_box=max_box,
             counts=(C.c_int32 * n)(*[v[0] for v in levels]), ratios=(C.c_float * n)(*[v[1] for v in levels]), n_levels=n, max_level=max_level,
             depth_scale=depth_scale, ws=p(ws), ws_bytes=need)
    a.update({k: p(v) for k, v in out.items()})
    a.update(over)
    torch.cuda.synchronize()                                                        # the uploads and fills above, whatever the stream
    rc = lib.parq_snippet_targets(*a.values(), C.c_void_p(stream.cuda_stream) if stream is not None else _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the call wrote behind its workspace"
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["sym"] = res.pop("sym_out")
    if fill is None or rc == 0:
        res["valid"] = res["valid"] != 0
    return rc, res


@pytest.mark.parametrize("c", SC.CASES, ids=IDS)
def test_module_equals_the_statement_and_the_fixture(c):
    got, want, p = run_module(c), statement(c), c["name"] + "/"
    assert_equals_statement(got, want, c["name"])
    for key in ("frame_points", "points_inside", "difficulty", "valid", "num_valid", "sym"):
        assert np.array_equal(got[key], Z[p + key]), key
    assert np.array_equal(got["obbs_padded"].view(np.uint32), Z[p + "obbs_padded"].view(np.uint32))
    for key in ("frame_truncation", "truncation"):
        err = SC.parity(got[key], Z[p + key])
        print("%s %s: parity to the fixture %.3e" % (c["name"], key, err))
        assert err <= 1e-4


@pytest.mark.parametrize("c", SC.CASES, ids=IDS)
def test_c_abi_equals_the_statement(c):
    rc, got = abi_call(SC.make_case(c))
    assert rc == 0
    assert_equals_statement(got, statement(c), c["name"])


@pytest.mark.parametrize("v", SC.LEVEL_VARIANTS, ids=[v["case"] for v in SC.LEVEL_VARIANTS])
def test_other_thresholds_and_max_box(v):
    c = SC.case_by_name(v["case"])
    kw = dict(levels=v["levels"], max_level=v["max_level"], max_box=v["max_box"])
    want = statement(c, **kw)
    assert_equals_statement(run_module(c, **kw), want, v["case"])
    rc, got = abi_call(SC.make_case(c), **kw)
    assert rc == 0
    assert_equals_statement(got, want, v["case"])


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_a_depth_buffer_at_any_2_byte_alignment(offset):
    """Frames that start 2, 4, 6 bytes past an 8-byte boundary and end anywhere: the first and the last word of the buffer are not
    wholly inside it.  The values around the frames are 0xFFFF (65.5 m): any of them read as a pixel shows up in a count."""
    c = SC.case_by_name("odd_61x77")
    d, args, _ = inputs(c)
    n = d["depth"].size
    host = np.full(offset + n + 7, 0xFFFF, np.uint16)
    host[offset:offset + n] = d["depth"].ravel()
    buf = torch.from_numpy(host).cuda()
    view = buf[offset:offset + n].view(d["depth"].shape)
    assert view.data_ptr() % 8 == 2 * offset and view.is_contiguous()
    args[0] = view
    assert_equals_statement(from_module(SnippetTargets()(*args, details=True)), statement(c), "offset %d" % offset)


def test_a_float32_pose_and_a_pose_wrapper_and_float32_corners():
    c = SC.case_by_name("six_digits")
    d, args, corners = inputs(c)
    base = from_module(SnippetTargets()(*args, details=True))                        # corners from the rows
    low = from_module(SnippetTargets()(*args, corners_world=corners.float(), details=True))
    assert_equals_statement(low, base, "float32 corners are not honoured: the rows are")
    M32 = d["T_world_camera"].astype(np.float32)
    d32 = dict(d, T_world_camera=M32.astype(np.float64), corners_world=None)
    Ki = np.stack([np.linalg.inv(K) for K in d["depth_intrinsics"]])
    want = SC.statement(d["depth"], Ki, d["color_intrinsics"], d["color_size"], d32["T_world_camera"], d["obbs"], d["sym"])
    args[4] = torch.from_numpy(M32).cuda()
    assert_equals_statement(from_module(SnippetTargets()(*args, details=True)), want, "float32 poses")
    args[4] = Pose.from_4x4mat(torch.from_numpy(M32))                                # a (B, T, 12) Pose on the CPU
    assert_equals_statement(from_module(SnippetTargets()(*args, details=True)), want, "Pose")


def test_results_do_not_depend_on_the_stream_or_on_what_runs_before():
    c = SC.case_by_name("levels_96x128")
    d, args, _ = inputs(c)
    want = statement(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = SnippetTargets()(*args, details=True)
    side.synchronize()
    assert_equals_statement(from_module(res), want, "side stream")
    rc, got = abi_call(d, stream=side)
    assert rc == 0
    assert_equals_statement(got, want, "C ABI on a side stream")
    # enqueued behind FramePrep on the same stream, no synchronisation in between
    B, T = c["B"], c["T"]
    frames = torch.randint(0, 256, (B, T, 37, 53, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    K = torch.from_numpy(d["color_intrinsics"][:, None, :3, :3].repeat(T, 1))
    with torch.cuda.stream(side):
        batch = F.FramePrep(size=(16, 12), pad=None)(frames, K, args[4])
        batch.update(SnippetTargets()(*args, details=True))
    side.synchronize()
    assert_equals_statement(from_module(batch), want, "behind FramePrep")
    assert sorted(batch)[:3] == ["T_camera_pseudoCam", "T_world_camera", "T_world_local"] and "rgb_img" in batch and "obbs_padded" in batch


def test_the_c_abi_refuses_each_argument_class_and_launches_nothing():
    lib = _lib.load()
    d = SC.make_case(SC.case_by_name("zero_frame"))
    odd = torch.zeros(d["depth"].size * 2 + 1, dtype=torch.uint8, device="cuda")
    bad = [dict(depth=None), dict(kinv=None), dict(kc=None), dict(poses=None), dict(obbs=None), dict(sym=None), dict(counts=None),
           dict(ratios=None), dict(ws=None), dict(obbs_padded=None), dict(sym_out=None), dict(num_valid=None), dict(frame_points=None),
           dict(frame_truncation=None), dict(points_inside=None), dict(truncation=None), dict(difficulty=None), dict(valid=None),
           dict(B=0), dict(B=1024), dict(T=0), dict(T=65), dict(Hd=0), dict(Wd=0), dict(Hd=8193), dict(Wd=8193), dict(N=0), dict(N=129),
           dict(color_h=0), dict(color_w=0), dict(color_h=8193), dict(color_w=8193), dict(max_box=0), dict(S=-1), dict(sym_is_int=2),
           dict(n_levels=0), dict(n_levels=9), dict(max_level=-1), dict(max_level=4), dict(depth_scale=0.0), dict(depth_scale=-1000.0),
           dict(depth_scale=float("nan")), dict(ws_bytes=15), dict(depth=C.c_void_p(odd.data_ptr() + 1))]
    for kw in bad:
        rc, got = abi_call(d, fill=113, **kw)
        assert rc == 1, kw                                                           # PARQ_ERR_ARG
        assert b"parq_snippet_targets" in lib.parq_last_error()
        for key, v in got.items():
            assert (v == 113).all(), ("a refused call launched something", kw, key)
    ws = torch.zeros(32, dtype=torch.uint8, device="cuda")
    rc, _ = abi_call(d, fill=113, ws=C.c_void_p(ws.data_ptr() + 8))
    assert rc == 1 and b"16-byte" in lib.parq_last_error()
    rc, got = abi_call(d, fill=113)
    assert rc == 0
    assert_equals_statement(got, statement(SC.case_by_name("zero_frame")), "after the refusals")


def test_the_module_refuses_cpu_depth_and_what_the_library_would():
    c = SC.case_by_name("zero_frame")
    _, args, _ = inputs(c)
    with pytest.raises(ValueError, match="SnippetTargets"):
        SnippetTargets()(args[0][:, :, :, ::2], *args[1:])
    with pytest.raises(RuntimeError, match="no CPU"):
        SnippetTargets()(args[0].cpu(), *args[1:])


# ---- FramePrep + SnippetTargets -> decoder.loss ------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [False, True], ids=["host_matcher", "match_on_device"])
def test_a_prepared_batch_goes_through_the_loss_like_the_statements_targets(on):
    c = SC.case_by_name("levels_96x128")
    d, args, _ = inputs(c)
    B, T = c["B"], c["T"]
    frames = torch.randint(0, 256, (B, T, 37, 53, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    K = torch.from_numpy(d["color_intrinsics"][:, None, :3, :3].repeat(T, 1))
    batch = F.FramePrep(size=(16, 12), pad=None)(frames, K, args[4])
    batch.update(SnippetTargets()(*args))
    assert sorted(batch) == ["T_camera_pseudoCam", "T_world_camera", "T_world_local", "T_world_pseudoCam", "camera", "num_valid", "obbs_padded",
                             "rgb_img", "sym"]
    want = statement(c)
    assert want["num_valid"].min() > 0

    cfg = synth.decoder_cfg(dim=256, queries=64, heads=4, ffn=256, layers=2, dropout=0.0)
    dec = make_decoder(cfg, synth.make_decoder_weights(cfg, 4300, damped=True)).train()
    dec.match_on_device = on
    sc = synth.make_scene(4301, B, T, 6, 8, 256)
    tokens, camera = torch.from_numpy(sc["tokens"]).cuda(), torch.from_numpy(sc["camera"]).cuda()

    def terms(obbs_padded, sym):
        np.random.seed(7)
        torch.manual_seed(7)
        dec._match_step = 0
        outs = dec(tokens, camera, batch["T_camera_pseudoCam"]._data, batch["T_world_pseudoCam"]._data, batch["T_world_local"]._data)
        res = dec.loss(outs, obbs_padded, batch["T_world_local"], sym)
        torch.cuda.synchronize()
        return {k: res[k].detach().cpu() for k in res if torch.is_tensor(res[k])}

    got = terms(batch["obbs_padded"], batch["sym"])
    ref = terms(Obb3D(torch.from_numpy(want["obbs_padded"].copy()).cuda()), torch.from_numpy(want["sym"].copy()).cuda())
    assert set(got) == set(ref) and "total_loss" in got
    for k in got:
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], ref[k]), k
