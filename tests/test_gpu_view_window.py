"""GPU tier: the streaming view window (parq_amd.ViewWindow, include/parq_hip.h parq_forward_views; INTEGRATION.md "Streaming a
window of views").  A window re-projects K / V of the view slots that were replaced since its last forward only; everything else of
the forward runs as always.  The claim tested here is bit equality (torch.equal on all six outputs of every iteration) with
``PARQDecoder.forward`` on the assembled inputs: the same kernels see the same rows, so no tolerance is involved.

Shapes (B = 2, V = 4, Q = 32, d = 256 / 4 heads / ffn 768 unless said otherwise; 2 iterations):
  8x8    64 keys per view: one 64-row tile of the persistent projection kernel per view
  16x16  256 keys per view: whole tiles
  5x20   100 keys per view, N = 400: views that start and end inside a tile (widening into both neighbours), the ragged path of mode
         "split" ("split8" runs as "split" here, as documented)
  big    8x8 at d = 1024 / 4 heads (head dim 256, the C > 256 kernel), B = 1, V = 3, Q = 16: ranges in 32-key cache blocks
The default policy ("sync") is live throughout: where the peakedness guard of mode "split8" trips on these small key counts the
window's forward is re-run with the heads moved, like any forward, and the reference decoder is put into the same ``safe_heads``."""
import ctypes as C
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from parq_amd import _lib, synth
from parq_amd.view_window import row_ranges
from gpu_util import make_decoder, dev

pytestmark = pytest.mark.gpu

KEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d", "sem_cls_prob", "coord_pos")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"8x8": (2, 4, 8, 8, 256), "16x16": (2, 4, 16, 16, 256), "5x20": (2, 4, 5, 20, 256), "big": (1, 3, 8, 8, 1024)}
MODES = ["split8", "split", "fp16", "bf16", "fp32"]
WQ = "parq_module.decoder.layers.0.multihead_attn.in_proj_weight"
# with the seeded weights as they are, 1024 keys are too few for the peakedness guard of mode "split8" (a row's probabilities relative to
# its maximum must sum to 256): it moves every head and the stage cache is never written.  Query rows of the cross-attention
# in-projection x 0.1 give rows that spread over all keys, so the tests of the stage-cache (and mixed-tier) projection run what they name
CALM = 0.1


@functools.lru_cache(maxsize=None)
def _model(dim, wq_scale=1.0):
    cfg = synth.decoder_cfg(dim=dim, queries=16 if dim == 1024 else 32, heads=4, ffn=768, layers=2)
    W = synth.make_decoder_weights(cfg, 6100 + dim, damped=True)
    if wq_scale != 1.0:
        W = dict(W)
        w = W[WQ].copy()
        w[:w.shape[1]] *= wq_scale                      # the query rows of the cross-attention in-projection (fixture g21's recipe)
        W[WQ] = w
    return cfg, W


@functools.lru_cache(maxsize=None)
def _scene(seed, shape, dtype=torch.float32):
    B, V, h, w, Cd = SHAPES[shape]
    sc = synth.make_scene(seed, B, V, h, w, Cd)
    return {k: dev(v).to(dtype) if k == "tokens" else dev(v) for k, v in sc.items()}


def _quiet(fn, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.no_grad():
            out = fn(*a, **k)
    return out


def _clone(outs):
    out = [{k: o[k].clone() for k in KEYS} for o in outs]
    torch.cuda.synchronize()
    return out


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in KEYS)


def _decoder(dim, mode, wq_scale=1.0, **settings):
    cfg, W = _model(dim, wq_scale)
    dec = make_decoder(cfg, W).eval()
    dec.attention_mode = mode
    dec._test_wq = wq_scale
    for k, v in settings.items():
        setattr(dec, k, v)
    return dec


def _fresh_like(dec, dim, wq_scale=None):
    """A fresh decoder with the same weights and settings (the head tiers a guard moved included)."""
    ref = _decoder(dim, dec.attention_mode, dec._test_wq if wq_scale is None else wq_scale, safe_heads=dec.safe_heads, range_check=dec.range_check,
                   batch_invariant=dec.batch_invariant, fuse_seams=dec.fuse_seams)
    ref.use_graph = False
    return ref


class _Inputs:
    """The assembled inputs of a window: scene `base` with slots replaced from other seeds, in one fixed local frame."""

    def __init__(self, shape, seed, dtype=torch.float32):
        self.shape, self.dtype = shape, dtype
        self.B, self.V, self.h, self.w, self.C = SHAPES[shape]
        self.t = {k: v.clone() for k, v in _scene(seed, shape, dtype).items()}

    def slot_rows(self, seed, slots):
        o = _scene(seed, self.shape, self.dtype)
        hw = self.h * self.w
        tok = o["tokens"].view(self.B, self.V, hw, self.C)[:, slots].contiguous()
        return tok, o["camera"][:, slots].contiguous(), o["T_camera_pseudoCam"][:, slots].contiguous(), o["T_world_pseudoCam"][:, slots].contiguous()

    def replace(self, win, seed, slots):
        tok, cam, T_cp, T_wp = self.slot_rows(seed, slots)
        hw = self.h * self.w
        self.t["tokens"].view(self.B, self.V, hw, self.C)[:, slots] = tok
        self.t["camera"][:, slots] = cam
        self.t["T_camera_pseudoCam"][:, slots] = T_cp
        self.t["T_world_pseudoCam"][:, slots] = T_wp
        win.put(slots if len(slots) > 1 else slots[0], tok if len(slots) > 1 else tok.view(self.B, hw, self.C), cam, T_cp, T_wp)

    def fill(self, win):
        allv = list(range(self.V))
        win.put(allv, self.t["tokens"], self.t["camera"], self.t["T_camera_pseudoCam"], self.t["T_world_pseudoCam"])

    def plain(self, dec):
        t = self.t
        return _clone(_quiet(dec, t["tokens"], t["camera"], t["T_camera_pseudoCam"], t["T_world_pseudoCam"], t["T_world_local"],
                             feat_hw=(self.h, self.w)))

    def window(self, dec):
        return dec.view_window(self.B, self.V, self.h, self.w, self.t["T_world_local"], dtype=self.dtype)


def _tile(shape):
    return 32 if shape == "big" else 64


def _check_rows(win, inp, slots, mode):
    N, hw = inp.V * inp.h * inp.w, inp.h * inp.w
    assert win.last_projected_views == sorted(slots)
    if mode == "fp32":
        # INTEGRATION.md "Streaming a window of views": attention mode "fp32" keeps no cache addressed by key and projects every row
        assert win.last_projected_rows == N
        doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
        assert 'mode `"fp32"` projects all `V*h*w` rows' in doc
        return
    runs = row_ranges(slots, inp.V, hw, _tile(inp.shape))
    rows = sum(b - a for a, b in runs)
    print("\n%s %s slots %s: projected %d of %d rows (dirty %d)" % (inp.shape, mode, slots, win.last_projected_rows, N, len(slots) * hw))
    assert win.last_projected_rows < N
    assert win.last_projected_rows <= len(slots) * hw + 2 * _tile(inp.shape) * len(runs)      # at most one tile / stage on each side of a run
    assert win.last_projected_rows == rows


def _step_equals_fresh(win, dec, inp, mode, seed, slots):
    inp.replace(win, seed, slots)
    got = _clone(_quiet(win.forward))
    _check_rows(win, inp, slots, mode)
    ref = _fresh_like(dec, inp.C)
    want = inp.plain(ref)
    assert ref.safe_heads == dec.safe_heads and ref.attention_mode == dec.attention_mode
    assert _same(got, want), (inp.shape, mode, slots)
    return got


def test_the_plain_forward_is_bit_reproducible_from_run_to_run():
    """What every comparison below rests on: a failure here is not a failure of the window."""
    for shape in SHAPES:
        inp = _Inputs(shape, 6201)
        dec = _decoder(inp.C, "split")
        a, b = inp.plain(dec), inp.plain(dec)
        assert _same(a, b), shape
        assert _same(a, inp.plain(_fresh_like(dec, inp.C))), shape


# 1 + 2: fill, one slot, two runs, one merged run, three consecutive steps
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fill_then_replaced_slots_equal_the_plain_forward_of_a_fresh_decoder(shape, mode):
    inp = _Inputs(shape, 6211)
    dec = _decoder(inp.C, mode)
    win = inp.window(dec)
    inp.fill(win)
    got = _clone(_quiet(win.forward))
    assert win.last_projected_views == list(range(inp.V)) and win.last_projected_rows == inp.V * inp.h * inp.w
    assert _same(got, inp.plain(_fresh_like(dec, inp.C)))
    last = inp.V - 1
    _step_equals_fresh(win, dec, inp, mode, 6212, [2])
    _step_equals_fresh(win, dec, inp, mode, 6213, [0, last])            # two runs
    _step_equals_fresh(win, dec, inp, mode, 6214, [1, 2])               # one merged run
    for k, slot in enumerate([1, 0, last]):                             # no stale row survives a sequence
        _step_equals_fresh(win, dec, inp, mode, 6215 + k, [slot])
    win.close()


# 3
@pytest.mark.parametrize("mode", ["split8", "fp32"])
def test_a_forward_with_nothing_dirty_projects_no_row_and_equals_the_one_before(mode):
    inp = _Inputs("16x16", 6221)
    dec = _decoder(inp.C, mode)
    win = inp.window(dec)
    inp.fill(win)
    _quiet(win.forward)                                   # (settles the tiers where the guard trips)
    first = _clone(_quiet(win.forward))
    second = _clone(_quiet(win.forward))
    assert win.last_projected_views == [] and win.last_projected_rows == 0
    assert _same(first, second) and _same(second, inp.plain(_fresh_like(dec, inp.C)))


# 4
def test_mixed_head_tiers():
    inp = _Inputs("16x16", 6231)
    dec = _decoder(inp.C, "split8", wq_scale=CALM, safe_heads=0b0101)
    win = inp.window(dec)
    inp.fill(win)
    got = _clone(_quiet(win.forward))
    print("\nmixed tiers: safe_heads after the fill = %s" % bin(dec.safe_heads))
    assert dec.safe_heads & 0b0101 == 0b0101
    assert dec.safe_heads == 0b0101, "the guard moved heads: the mixed-tier (stage + split layout) projection is not what runs"
    assert win.last_projected_views == [0, 1, 2, 3] and _same(got, inp.plain(_fresh_like(dec, inp.C)))
    _step_equals_fresh(win, dec, inp, "split8", 6232, [2])
    _step_equals_fresh(win, dec, inp, "split8", 6233, [0, 3])


# 5
def test_every_state_change_projects_all_slots_again():
    inp = _Inputs("16x16", 6241)
    dec = _decoder(inp.C, "split8")
    win = inp.window(dec)
    inp.fill(win)
    _quiet(win.forward)
    _quiet(win.forward)
    assert win.last_projected_views == []

    def changed(what):
        got = _clone(_quiet(win.forward))
        assert win.last_projected_views == [0, 1, 2, 3], what
        ref = _fresh_like(dec, inp.C)
        with torch.no_grad():
            ref.load_state_dict(dec.state_dict())
        assert _same(got, inp.plain(ref)), what
        _quiet(win.forward)
        assert win.last_projected_views == [], what
    with torch.no_grad():
        for p in dec.parq_module.decoder.layers[0].multihead_attn.parameters():
            p.add_(0.01)                                  # an optimizer-style in-place update of the K/V projection's own weights
    changed("weights")
    dec.attention_mode = "split"
    changed("attention_mode")
    dec.attention_mode = "split8"
    changed("attention_mode back")
    dec.safe_heads = dec.safe_heads ^ 0b0010 if dec.safe_heads != 0b1111 else 0b1101
    changed("safe_heads")
    dec.batch_invariant = True
    changed("batch_invariant")


# 6
def test_sync_policy_never_returns_nan_and_reruns_with_what_the_fallback_changed():
    inp = _Inputs("16x16", 6251)
    dec = _decoder(inp.C, "split8", wq_scale=4.0)
    assert dec.range_check == "sync"
    win = inp.window(dec)
    inp.fill(win)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad():
            got = _clone(win.forward())
    assert dec.safe_heads != 0 and any("too few keys" in str(w.message) for w in caught), "the x 4 fixture is meant to trip the guard"
    assert win.last_projected_views == [0, 1, 2, 3]
    assert all(torch.isfinite(o[k]).all() for o in got for k in KEYS)
    assert _same(got, inp.plain(_fresh_like(dec, inp.C, 4.0)))
    inp.replace(win, 6252, [1])
    got = _clone(_quiet(win.forward))
    assert all(torch.isfinite(o[k]).all() for o in got for k in KEYS)
    ref = _fresh_like(dec, inp.C, 4.0)                     # (in the FINAL safe_heads: a head this step moved is moved there too)
    assert _same(got, inp.plain(ref)) and ref.safe_heads == dec.safe_heads


def test_lazy_policy_a_flagged_forward_leaves_all_slots_dirty():
    inp = _Inputs("16x16", 6261)
    dec = _decoder(inp.C, "split", range_check="lazy")
    win = inp.window(dec)
    inp.fill(win)
    _quiet(win.forward)
    torch.cuda.synchronize()
    assert win.dirty_slots == []
    tok, cam, T_cp, T_wp = inp.slot_rows(6262, [1])
    tok = tok * 3e4                                       # beyond the fp16 range: the projection raises the range flag
    inp.t["tokens"].view(inp.B, inp.V, -1, inp.C)[:, [1]] = tok
    inp.t["camera"][:, [1]], inp.t["T_camera_pseudoCam"][:, [1]], inp.t["T_world_pseudoCam"][:, [1]] = cam, T_cp, T_wp
    win.put(1, tok.view(inp.B, -1, inp.C), cam, T_cp, T_wp)
    got = _clone(_quiet(win.forward))
    assert win.last_projected_views == [1]
    assert torch.isnan(got[0]["pred_logits"]).all() and torch.isnan(got[-1]["ortho6d"]).all(), "never wrong numbers: the flagged forward is NaN"
    assert win.dirty_slots == [0, 1, 2, 3]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad():
            got = _clone(win.forward())                   # the next call polls, switches to "fp32" and projects everything
    assert dec.attention_mode == "fp32" and any("fp16 range" in str(w.message) for w in caught)
    assert win.last_projected_views == [0, 1, 2, 3] and all(torch.isfinite(o[k]).all() for o in got for k in KEYS)
    assert _same(got, inp.plain(_fresh_like(dec, inp.C)))


# 7
def test_the_third_forward_replays_the_graph_and_equals_the_uncaptured_window():
    inp_a, inp_b = _Inputs("16x16", 6271), _Inputs("16x16", 6271)
    dec_a, dec_b = _decoder(256, "split"), _decoder(256, "split")
    dec_b.use_graph = False
    win_a, win_b = inp_a.window(dec_a), inp_b.window(dec_b)
    inp_a.fill(win_a)
    inp_b.fill(win_b)
    for k in range(4):
        if k:
            inp_a.replace(win_a, 6272 + k, [k % 4])
            inp_b.replace(win_b, 6272 + k, [k % 4])
        before = win_a._entry.replays if win_a._entry is not None else 0
        a, b = _clone(_quiet(win_a.forward)), _clone(_quiet(win_b.forward))
        assert _same(a, b), k
        assert win_a.last_projected_views == win_b.last_projected_views == ([0, 1, 2, 3] if k == 0 else [k % 4])
        if k >= 2:
            assert win_a._entry.replays == before + 1, "from the second forward of a key on the iterations replay"
    assert win_b._entry.replays == 0
    assert dec_a._ws == {} and dec_b._ws == {}, "the window's workspace lives outside the max_workspaces cache"


# 8
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", ["5x20", "big", "16x16", "16x16-mixed"])
def test_16_bit_windows_read_their_tokens_natively(shape, dtype):
    """5x20 runs as "split", big is the C > 256 kernel; 16x16 is the stage cache of mode "split8" (all heads on the fast tier, or
    heads 0 and 2 on the fp16 x 3 tier: the mixed projection) read from 16-bit tokens over a row range."""
    shape, mixed = (shape.split("-")[0], True) if "-" in shape else (shape, False)
    inp = _Inputs(shape, 6281, dtype)
    dec = _decoder(inp.C, "split8", wq_scale=CALM if shape == "16x16" else 1.0, safe_heads=0b0101 if mixed else 0)
    win = inp.window(dec)
    assert win.tokens.dtype == dtype
    inp.fill(win)
    got = _clone(_quiet(win.forward))
    if shape == "16x16":
        print("\n16-bit %s: safe_heads after the fill = %s" % ("mixed" if mixed else "fast", bin(dec.safe_heads)))
        assert dec.safe_heads == (0b0101 if mixed else 0), "the guard moved heads: the stage-cache projection is not what runs"
    assert _same(got, inp.plain(_fresh_like(dec, inp.C)))
    _step_equals_fresh(win, dec, inp, "split8", 6282, [2])
    _step_equals_fresh(win, dec, inp, "split8", 6283, [0, 1])


# 9
def test_view_mass_after_a_window_forward_is_the_plain_forwards():
    inp = _Inputs("16x16", 6291)
    dec = _decoder(inp.C, "split")
    win = inp.window(dec)
    inp.fill(win)
    _quiet(win.forward)
    inp.replace(win, 6292, [3])
    _quiet(win.forward)
    got = dec.cross_attention_view_mass().clone()
    gmap = dec.cross_attention_map(queries=[0, 5]).clone()
    ref = _fresh_like(dec, inp.C)
    inp.plain(ref)
    assert torch.equal(got, ref.cross_attention_view_mass()) and got.shape == (inp.B, 32, inp.V)
    assert torch.equal(gmap, ref.cross_attention_map(queries=[0, 5]))


# 10
def test_rebase_makes_every_slot_dirty_and_unput():
    inp = _Inputs("8x8", 6301)
    dec = _decoder(inp.C, "split")
    win = inp.window(dec)
    inp.fill(win)
    _quiet(win.forward)
    new = _Inputs("8x8", 6302)
    win.rebase(new.t["T_world_local"])
    new.replace(win, 6302, [0, 1])
    with pytest.raises(RuntimeError, match="have not been put"):
        win.forward()
    new.replace(win, 6302, [2, 3])
    got = _clone(_quiet(win.forward))
    assert win.last_projected_views == [0, 1, 2, 3]
    assert _same(got, new.plain(_fresh_like(dec, inp.C)))
    assert torch.equal(win.T_world_local.view(-1), new.t["T_world_local"].view(-1))


# 11
@pytest.mark.parametrize("hw", [(8, 8), (16, 16), (5, 20)], ids=["8x8", "16x16", "5x20"])
@pytest.mark.parametrize("pyramid", [False, True], ids=["features", "pyramid"])
def test_module_level_window_encodes_the_put_views_only(hw, pyramid):
    from types import SimpleNamespace as NS
    from parq_amd import PARQ, Camera, Pose
    B, V, Cd, (h, w) = 2, 4, 256, hw
    dcfg = synth.decoder_cfg(dim=Cd, queries=32, heads=4, ffn=768, layers=2)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg))
    model = PARQ(cfg).eval()
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
    cam, T_cp, T_wp, T_wl = (dev(a) for a in synth.make_geometry(6313, B, V, h, w))
    if pyramid:
        sizes = [(h, w), (max(2, h // 2), max(2, w // 2)), (max(2, h // 4), max(2, w // 4)), (max(2, h // 4), max(2, w // 4))]
        feats = [dev(synth.normal(6314 + i, "lv", (B, V, Cd // 4, s[0], s[1]), std=0.5)) for i, s in enumerate(sizes)]
        pick = lambda sl: ([f[:, sl].contiguous() for f in feats], 0)
        batch = {"fpn_features": feats, "fpn_layer": 0}
    else:
        feats = dev(synth.normal(6314, "feat", (B, V, Cd, h, w), std=0.5))
        pick = lambda sl: feats[:, sl].contiguous()
        batch = {"all_features": feats}
    batch.update({"camera_feature": Camera(cam), "T_camera_pseudoCam": Pose(T_cp), "T_world_pseudoCam": Pose(T_wp), "T_world_local": Pose(T_wl)})
    with torch.no_grad():
        if pyramid:
            want_tok = model.add_ray_pe.tokens_from_pyramid(feats, 0, cam, T_cp, T_wp, T_wl).clone()
        else:
            want_tok = model.add_ray_pe.tokens(feats, cam, T_cp, T_wp, T_wl).clone()
        want = _clone(model(batch, 0)[1])
    win = model.view_window(B, V, h, w, T_wl)
    for sl in ([0], [1, 2], [3]):
        win.put_features(sl if len(sl) > 1 else sl[0], pick(sl), Camera(cam[:, sl]), Pose(T_cp[:, sl]), Pose(T_wp[:, sl]))
    torch.cuda.synchronize()
    assert torch.equal(win.tokens, want_tok), "a view's tokens do not depend on which views are encoded with it"
    got = _clone(_quiet(win.forward))
    assert _same(got, want)
    win.put_features(2, pick([2]), Camera(cam[:, [2]]), Pose(T_cp[:, [2]]), Pose(T_wp[:, [2]]))
    assert torch.equal(win.tokens, want_tok)
    got = _clone(_quiet(win.forward))
    assert win.last_projected_views == [2] and _same(got, want)


# 12
def test_the_c_abi_directly():
    inp = _Inputs("5x20", 6321)
    dec = _decoder(inp.C, "split", range_check="off")
    dec.use_graph = False
    want = inp.plain(dec)
    lib, h = _lib.load(), dec._handle()
    t = inp.t
    sc, keep, dev_ = dec._scene(t["tokens"], t["camera"], t["T_camera_pseudoCam"], t["T_world_pseudoCam"], t["T_world_local"], (inp.h, inp.w))
    nbytes = lib.parq_workspace_bytes(h, sc.B, sc.V, sc.h, sc.w)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev_)                # a workspace the library has never seen
    outs = dec._alloc_outputs((dec.num_layers, sc.B, dec.num_queries), dev_)
    po = _lib.ParqOutputs(*[_lib.ptr(o) for o in outs])
    rows = C.c_int64(-1)

    def call(views, graph=None):
        arr = (C.c_int32 * max(1, len(views)))(*views)
        rc = lib.parq_forward_views(h, graph, C.byref(sc), _lib.ptr(ws), ws.numel() * 4, C.byref(po), arr, len(views), C.byref(rows),
                                    _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc

    def equal_want(w):
        return all(torch.equal(outs[i][k], w[k][key]) for i, key in enumerate(KEYS) for k in range(dec.num_layers))
    N = inp.V * inp.h * inp.w
    assert call([1]) == 3 and b"never filled" in lib.parq_last_error()                  # PARQ_ERR_STATE
    assert call([0, 1, 2, 4]) == 1 and b"outside" in lib.parq_last_error()              # PARQ_ERR_ARG: index V
    assert call([0, 2, 2]) == 1 and b"twice" in lib.parq_last_error()                   # PARQ_ERR_ARG: a duplicate
    assert call([3, 1, 0, 2]) == 0 and rows.value == N and equal_want(want)             # all views, any order: parq_forward
    # one slot replaced in the caller's token buffer
    tok, cam, T_cp, T_wp = inp.slot_rows(6322, [2])
    inp.t["tokens"].view(inp.B, inp.V, -1, inp.C)[:, [2]] = tok
    inp.t["camera"][:, [2]], inp.t["T_camera_pseudoCam"][:, [2]], inp.t["T_world_pseudoCam"][:, [2]] = cam, T_cp, T_wp
    assert call([2]) == 0
    assert rows.value == sum(b - a for a, b in row_ranges([2], inp.V, inp.h * inp.w, 64)) == 128 and rows.value < N
    assert equal_want(inp.plain(_fresh_like(dec, inp.C)))
    assert call([]) == 0 and rows.value == 0 and equal_want(inp.plain(_fresh_like(dec, inp.C)))
    # with a captured graph
    g = C.c_void_p()
    _lib.check(lib.parq_forward_capture(h, sc.B, sc.V, sc.h, sc.w, _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr(), C.byref(g)), "capture")
    assert call([0, 3], g) == 0 and rows.value == 128 + 144 and equal_want(inp.plain(_fresh_like(dec, inp.C)))
    # the attention mode changed since the cache was built
    _lib.check(lib.parq_set_attention_mode(h, 2), "mode")
    assert call([2]) == 3 and b"attention mode" in lib.parq_last_error()
    _lib.check(lib.parq_set_attention_mode(h, 1), "mode")
    assert call([2]) == 0
    # parq_prepare hands the workspace to a stepping driver: the record is gone
    _lib.check(lib.parq_prepare(h, C.byref(sc), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()), "prepare")
    assert call([2]) == 3
    assert lib.parq_graph_destroy(g) == 0


def test_a_subset_call_keeps_the_range_flag_of_the_forward_that_projected_the_skipped_rows():
    """The host's look at the mirror word cannot see a flag that a forward still in flight is about to raise.  The device keeps it: a
    call that skips rows does not clear the workspace's range flag, so it is poisoned (NaN) like the forward that projected the
    overflowed rows, and only a call that lists all views clears the flag.  Shown without a race, through the C ABI with NO mirror word
    set (the host check then does not exist at all)."""
    inp = _Inputs("16x16", 6331)
    dec = _decoder(inp.C, "split", range_check="off")
    dec.use_graph = False
    inp.plain(dec)                                          # packs the weights
    lib, h = _lib.load(), dec._handle()
    t = inp.t
    sc, keep, dev_ = dec._scene(t["tokens"], t["camera"], t["T_camera_pseudoCam"], t["T_world_pseudoCam"], t["T_world_local"], (inp.h, inp.w))
    ws = torch.empty(lib.parq_workspace_bytes(h, sc.B, sc.V, sc.h, sc.w) // 4, dtype=torch.float32, device=dev_)
    outs = dec._alloc_outputs((dec.num_layers, sc.B, dec.num_queries), dev_)
    po = _lib.ParqOutputs(*[_lib.ptr(o) for o in outs])

    def call(views):
        arr = (C.c_int32 * max(1, len(views)))(*views)
        rc = lib.parq_forward_views(h, None, C.byref(sc), _lib.ptr(ws), ws.numel() * 4, C.byref(po), arr, len(views), None, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    nan = lambda: bool(torch.isnan(outs[0][0]).all() and torch.isnan(outs[3][-1]).all())
    _lib.check(lib.parq_set_range_mirror(h, None), "mirror off")
    try:
        good = t["tokens"].view(inp.B, inp.V, -1, inp.C)[:, 1].clone()
        t["tokens"].view(inp.B, inp.V, -1, inp.C)[:, 1] *= 3e4          # slot 1 beyond the fp16 range
        assert call([0, 1, 2, 3]) == 0 and nan()
        assert call([3]) == 0 and nan(), "slot 1's overflowed rows are still in the cache"
        assert call([]) == 0 and nan()
        t["tokens"].view(inp.B, inp.V, -1, inp.C)[:, 1] = good
        assert call([1]) == 0 and nan(), "only a call that lists all views clears the flag"
        assert call([0, 1, 2, 3]) == 0 and not nan() and all(bool(torch.isfinite(o).all()) for o in outs)
        assert call([2]) == 0 and all(bool(torch.isfinite(o).all()) for o in outs)
    finally:
        _lib.check(lib.parq_set_range_mirror(h, C.c_void_p(dec._mirror_ptr(0))), "mirror on")
        dec._mirror_set = 0


def test_a_plain_forward_that_polls_the_windows_word_leaves_the_window_all_dirty():
    """range_check = "off": no fallback changes the state, so the window only learns of its flagged forward from its mirror word —
    also when a plain decoder.forward in between is the one that takes it."""
    inp = _Inputs("16x16", 6341)
    dec = _decoder(inp.C, "split", range_check="off")
    win = inp.window(dec)
    inp.fill(win)
    _quiet(win.forward)
    tok, cam, T_cp, T_wp = inp.slot_rows(6342, [1])
    win.put(1, (tok * 3e4).view(inp.B, -1, inp.C), cam, T_cp, T_wp)
    _clone(_quiet(win.forward))                             # raises the window's word
    assert win.last_projected_views == [1] and win.dirty_slots == [0, 1, 2, 3]
    inp.plain(dec)                                          # a plain forward of the same decoder polls (and clears) every word
    assert win.dirty_slots == [0, 1, 2, 3]
    _quiet(win.forward)
    assert win.last_projected_views == [0, 1, 2, 3]


def test_a_subset_the_library_refuses_is_enqueued_again_with_all_views():
    """The window compares the keys the library records, so PARQ_ERR_STATE is not expected; where it still comes (here: the record
    dropped behind the window's back by parq_prepare in its workspace) the forward is enqueued with every view, not raised."""
    inp = _Inputs("8x8", 6351)
    dec = _decoder(inp.C, "split")
    win = inp.window(dec)
    inp.fill(win)
    _quiet(win.forward)
    ws = win._entry.ws
    _lib.check(_lib.load().parq_prepare(dec._handle(), C.byref(win._sc), _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr()), "prepare")
    inp.replace(win, 6352, [2])
    got = _clone(_quiet(win.forward))
    assert win.last_projected_views == [0, 1, 2, 3] and win.last_projected_rows == inp.V * inp.h * inp.w
    assert _same(got, inp.plain(_fresh_like(dec, inp.C)))
    _step_equals_fresh(win, dec, inp, "split", 6353, [1])
