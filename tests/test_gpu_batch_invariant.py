"""GPU tier: batch-invariant inference (PARQDecoder.batch_invariant; include/parq_hip.h parq_set_batch_invariant).

By default the launch geometry follows the call — key-split counts of both attentions (ceil(CUs / (B * heads * query tiles))), 16- or
32-row tiles of the chain GEMMs, the slots that collect the heads' GroupNorm moments — so a scene's outputs differ in the last bits with
the number of scenes that share its forward.  With the flag every such choice is made as for ONE scene.  Contract tested here, always
with torch.equal on all six outputs of every iteration: scene i of a B-scene call under the flag returns the bits the DEFAULT path gives
that scene alone, at every position and in any company; the number of launches does not depend on B; a one-scene call under the flag
is the default call.  Every forward is also checked to be finite and to have raised no range / too-peaked flag (with the default
"sync" policy a flagged forward would be re-run under other arithmetic, which could hide a difference or cause one).

The shapes are the smallest at which the default code provably takes another geometry at B = 1 and B > 1 on a 256-CU device (the key
count large enough that the split pickers' cap, the number of key stages / tiles, does not bind at both)."""
import ctypes as C
import os
import re

import pytest
import torch

from parq_amd import _lib, synth
from gpu_util import dev, make_decoder, scene_args

pytestmark = pytest.mark.gpu

KEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d", "sem_cls_prob", "coord_pos")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERMS = {3: (2, 0, 1), 5: (3, 1, 4, 0, 2)}


def _gn_slots_constant():
    src = open(os.path.join(ROOT, "parq_amd", "csrc", "common.hpp")).read()
    return int(re.search(r"constexpr\s+int\s+kGnSlots\s*=\s*(\d+)\s*;", src).group(1))


def _cat(scenes, order):
    return tuple(torch.cat([scenes[i][j] for i in order]).contiguous() for j in range(5))


def _no_flags(dec):
    mode, safe = dec._expect
    assert not dec.fp16_range_exceeded(), "a range flag was raised"
    assert not dec.attention_too_peaked(), "the peakedness guard of mode split8 was raised"
    assert dec.safe_heads == safe and dec.attention_mode == mode, (dec.safe_heads, dec.attention_mode)


def _run(dec, args, hw):
    with torch.no_grad():
        out = [{k: o[k].clone() for k in KEYS} for o in dec(*args, feat_hw=hw)]
    torch.cuda.synchronize()
    assert all(torch.isfinite(o[k]).all() for o in out for k in KEYS)
    _no_flags(dec)
    return out


def _diff(batch_out, i, single_out):
    """Keys (iteration, name) in which scene i of the batch differs from the scene alone."""
    return [(k, key) for k, (b, s) in enumerate(zip(batch_out, single_out)) for key in KEYS if not torch.equal(b[key][i:i + 1], s[key])]


class _Case:
    """A decoder, n one-scene argument tuples and the DEFAULT path's outputs of every scene alone (computed once, shared)."""

    def __init__(self, dim, heads, Q, ffn, V, h, w, mode, n=5, seed=7100, safe=0, q_scale=None, layers=2):
        self.hw = (h, w)
        cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=heads, ffn=ffn, layers=layers)
        W = synth.make_decoder_weights(cfg, seed, damped=True)
        if q_scale is not None:
            # the cross-attention query projection scaled down: rows spread over the keys (the split8 guard looks at a row sum of 256)
            for name in list(W):
                if name.endswith("multihead_attn.in_proj_weight") or name.endswith("multihead_attn.in_proj_bias"):
                    W[name] = W[name].copy()
                    W[name][:dim] *= q_scale
        self.dec = make_decoder(cfg, W).eval()
        if mode:
            self.dec.attention_mode = mode
        self.dec.safe_heads = safe
        self.dec._expect = (self.dec.attention_mode, safe)
        self.scenes = [scene_args(synth.make_scene(seed + 11 * (i + 1), 1, V, h, w, dim, smooth=True)) for i in range(n)]
        self.dec.batch_invariant = False
        self.alone = [_run(self.dec, s, self.hw) for s in self.scenes]
        self.dec.batch_invariant = True

    def check(self, B):
        for order in (tuple(range(B)), PERMS[B]):
            got = _run(self.dec, _cat(self.scenes, order), self.hw)
            for pos, i in enumerate(order):             # first, middle, last — every position
                assert _diff(got, pos, self.alone[i]) == [], (order, pos)


_CASES = {}


def _case(key, **kw):
    if key not in _CASES:
        _CASES.clear()                                   # one case's modules and scenes alive at a time
        _CASES[key] = _Case(**kw)
    return _CASES[key]


# 1. d = 256, 4 heads, Q = 256, 2 views of 48 x 64 (6144 keys = 96 stages): 64 key splits at one scene, 22 at three, 13 at five
@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("mode", ["split", "fp16", "bf16", "fp32"])
def test_scene_in_a_batch_equals_the_scene_alone(mode, B):
    _case(("d256", mode), dim=256, heads=4, Q=256, ffn=768, V=2, h=48, w=64, mode=mode).check(B)


# 2. the same in mode split8 (guard down), and with two head sets of their own split counts
@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("safe", [0, 0b0101])
def test_scene_in_a_batch_equals_the_scene_alone_in_split8(safe, B):
    case = _case(("d256", "split8", safe), dim=256, heads=4, Q=256, ffn=768, V=2, h=48, w=64, mode="split8", safe=safe, q_scale=0.25)
    assert case.dec.attention_mode == "split8" and case.dec.safe_heads == safe
    case.check(B)
    low = case.dec.attention_min_row_sum()
    assert low is not None and low >= 256.0, low


# 3. ragged key count: 2 views of 47 x 63 = 5922 keys, no multiple of 64
def test_ragged_key_count():
    _case(("ragged",), dim=256, heads=4, Q=256, ffn=768, V=2, h=47, w=63, mode="split", n=3).check(3)


# 4. the shipped width: d = 1024, head dim 256, Q = 128, 2400 keys (75 blocks): 64 splits at one scene, 16 at three; M = 128 against 384
#    also moves the 32-row-tile decisions of the fp16 x 3 chain tile, and (Q / 16) (C / 16) = 512 sub-tiles exceed the default moment slots
def test_shipped_width():
    case = _case(("d1024",), dim=1024, heads=4, Q=128, ffn=768, V=1, h=30, w=40, mode="split", n=3)
    assert (128 // 16) * (1024 // 16) > _gn_slots_constant()
    case.check(3)


# 5. head dims 32 and 128 (the fp32 kernels; d = 128 / 512 run the generic GEMM kernel)
@pytest.mark.parametrize("dim,heads", [(256, 8), (128, 1), (512, 4)])
def test_head_dims_32_and_128(dim, heads):
    _case(("hd", dim, heads), dim=dim, heads=heads, Q=32, ffn=256, V=2, h=40, w=48, mode="fp32", n=3).check(3)


# 6. GroupNorm moments on both sides of the own-slot condition (rows per scene / 16) (group columns / 16) <= kGnSlots
@pytest.mark.parametrize("Q", [256, 272])
def test_groupnorm_moment_slots_on_both_sides_of_the_own_slot_condition(Q):
    slots = _gn_slots_constant()
    own = (Q // 16) * (256 // 16) <= slots
    assert own == (Q == 256), "one shape on each side of the condition"
    case = _case(("gn", Q), dim=256, heads=4, Q=Q, ffn=256, V=1, h=24, w=32, mode="fp32", n=3)
    # what the library carves: the default layout has kGnSlots slots per (scene, head); under the flag every sub-tile has its own
    dec, (h, w) = case.dec, case.hw
    off, n = C.c_size_t(), C.c_size_t()
    numel = {}
    for flag in (False, True):
        dec.batch_invariant = flag
        _lib.check(_lib.load().parq_workspace_lookup(dec._handle(), 3, 1, h, w, b"gn_sums_f64", C.byref(off), C.byref(n)), "lookup")
        numel[flag] = n.value // (2 * 3 * 4 * 2)
    assert numel[False] == slots
    assert numel[True] == (slots if own else ((Q // 16) * 16 + 63) // 64 * 64) and numel[True] >= (Q // 16) * 16
    case.check(3)


# 7. one scene: the flag changes nothing — bits and launches; under the flag the launch count does not depend on B
@pytest.mark.parametrize("shape", ["d256", "d1024"])
def test_one_scene_is_the_default_call_and_launches_do_not_depend_on_the_batch(shape):
    kw = (dict(dim=256, heads=4, Q=256, ffn=768, V=2, h=48, w=64, mode="split") if shape == "d256" else
          dict(dim=1024, heads=4, Q=128, ffn=768, V=1, h=30, w=40, mode="split"))
    case = _case(("one", shape), n=4, **kw)
    dec, hw = case.dec, case.hw

    def launches(flag, args):
        """(graph nodes of the captured iterations, bracketed launch groups of a profiled forward) — and the outputs of every call."""
        dec.batch_invariant = flag
        dec._ws.clear()                                         # a fresh workspace: its forwards are counted from zero
        outs = [_run(dec, args, hw) for _ in range(3)]          # direct, captured + replayed, replayed
        entry = next(reversed(dec._ws.values()))
        assert entry.replays == 2 and len(entry.graphs) == 1
        nodes = _lib.load().parq_graph_nodes(next(iter(entry.graphs.values())))
        dec.profile_enable(True)
        dec.profile_read()
        _run(dec, args, hw)                                     # (a profiled forward keeps pe1 and project + sample apart: other bits)
        groups = {k: v[1] for k, v in dec.profile_read().items()}
        dec.profile_enable(False)
        assert all(_diff(o, i, [{k: x[k][i:i + 1] for k in KEYS} for x in outs[0]]) == [] for o in outs[1:] for i in range(args[0].shape[0]))
        return nodes, groups, outs[0]
    off = launches(False, case.scenes[0])
    on = launches(True, case.scenes[0])
    assert _diff(on[2], 0, off[2]) == [] and _diff(on[2], 0, case.alone[0]) == []
    assert on[0] == off[0] and on[1] == off[1], (on[:2], off[:2])
    on4 = launches(True, _cat(case.scenes, (0, 1, 2, 3)))
    assert on4[0] == on[0] and on4[1] == on[1], (on4[:2], on[:2])
    assert on4[0] >= 8 * dec.num_layers
    for i in range(4):
        assert _diff(on4[2], i, case.alone[i]) == []


# 8. the captured forward under the flag, and toggling the flag between calls
def test_captured_forward_and_toggling_the_flag():
    case = _case(("graph",), dim=256, heads=4, Q=256, ffn=768, V=2, h=48, w=64, mode="split", n=3)
    dec, hw = case.dec, case.hw
    batch = _cat(case.scenes, (0, 1, 2))
    dec.use_graph = False
    want = {True: _run(dec, batch, hw)}
    dec.batch_invariant = False
    want[False] = _run(dec, batch, hw)
    assert any(_diff(want[False], i, case.alone[i]) for i in range(3)), "the default path is expected to depend on the batch at this shape"
    dec.use_graph = True
    replays = lambda: sum(e.replays for e in dec._ws.values())
    for flag in (True, False, True):
        dec.batch_invariant = flag
        for rep in range(3):                             # direct, capture + replay, replay — all three are this setting's forward
            got = _run(dec, batch, hw)
            assert all(_diff(got, i, [{k: o[k][i:i + 1] for k in KEYS} for o in want[flag]]) == [] for i in range(3)), (flag, rep)
        entry = next(reversed(dec._ws.values()))
        assert replays() == 2 and len(entry.graphs) == 1, "changing the flag dropped the workspaces: the forward was captured again"
        assert next(iter(entry.graphs))[-2] is flag, "the flag is part of the graph key"
    # the C ABI refuses a graph recorded under the other setting
    lib, h = _lib.load(), dec._handle()
    sc, keep, dev_ = dec._scene(*batch, feat_hw=hw)
    entry = next(reversed(dec._ws.values()))
    g = next(iter(entry.graphs.values()))
    outs = dec._alloc_outputs((dec.num_layers, sc.B, dec.num_queries), dev_)
    po = _lib.ParqOutputs(*[_lib.ptr(t) for t in outs])
    _lib.check(lib.parq_set_batch_invariant(h, 0), "flag")
    assert lib.parq_forward_replay(h, g, C.byref(sc), _lib.ptr(entry.ws), entry.ws.numel() * 4, C.byref(po), _lib.stream_ptr()) == 3
    assert b"capture again" in lib.parq_last_error()
    _lib.check(lib.parq_set_batch_invariant(h, 1), "flag")
    assert lib.parq_set_batch_invariant(h, 2) != 0
    torch.cuda.synchronize()


# 9. the other entry points: prepare + iterate, InFlight, the cross-attention maps
def test_prepare_iterate_inflight_and_attention_maps():
    from parq_amd import InFlight
    case = _case(("entry",), dim=256, heads=4, Q=256, ffn=768, V=2, h=48, w=64, mode="split", n=3)
    dec, hw = case.dec, case.hw
    batch = _cat(case.scenes, (1, 0, 2))                 # scene 0 in the middle

    def stepped(args):
        dec.prepare(*args, feat_hw=hw)
        outs = []
        for k in range(dec.num_layers):
            o, _ = dec.iterate(k)
            outs.append({key: o[key].clone() for key in KEYS})
        maps = (dec.cross_attention_map(queries=[0, 17, 255]).clone(), dec.cross_attention_view_mass().clone())
        torch.cuda.synchronize()
        assert all(torch.isfinite(o[k]).all() for o in outs for k in KEYS) and all(torch.isfinite(m).all() for m in maps)
        _no_flags(dec)
        return outs, maps
    one, maps1 = stepped(case.scenes[0])
    three, maps3 = stepped(batch)
    assert _diff(one, 0, case.alone[0]) == [], "prepare + iterate of one scene is the forward of that scene"
    assert _diff(three, 1, one) == []
    assert torch.equal(maps3[0][1:2], maps1[0]) and torch.equal(maps3[1][1:2], maps1[1])
    # after a forward too
    _run(dec, case.scenes[0], hw)
    m1 = (dec.cross_attention_map(per_head=True, queries=[3]).clone(), dec.cross_attention_view_mass().clone())
    _run(dec, batch, hw)
    m3 = (dec.cross_attention_map(per_head=True, queries=[3]).clone(), dec.cross_attention_view_mass().clone())
    torch.cuda.synchronize()
    assert torch.equal(m3[0][1:2], m1[0]) and torch.equal(m3[1][1:2], m1[1])
    # two forwards in flight on two streams: a one-scene and a three-scene call that share a scene
    with torch.no_grad():
        runner = InFlight(dec, depth=2)
        for rep in range(2):
            t1 = runner.submit(*case.scenes[0], feat_hw=hw)
            t3 = runner.submit(*batch, feat_hw=hw)
            g1, g3 = t1.result(), t3.result()
            torch.cuda.synchronize()
            for got in (g1, g3):
                assert all(torch.isfinite(o[k]).all() for o in got for k in KEYS)
            assert _diff(g1, 0, case.alone[0]) == [] and _diff(g3, 1, case.alone[0]) == [], rep
            assert _diff(g3, 0, case.alone[1]) == [] and _diff(g3, 2, case.alone[2]) == [], rep
        runner.drain()
    assert dec.safe_heads == 0 and dec.attention_mode == "split"


# 10. end to end: ray-PE tokenisation -> decoder -> parse_pred
def test_detections_of_a_scene_do_not_depend_on_the_batch():
    from types import SimpleNamespace as NS
    from parq_amd import PARQ, Camera, Pose
    from parq_amd.wrappers import raw
    _CASES.clear()
    V, h, w, Cd, Qn = 2, 48, 64, 256, 256
    dcfg = synth.decoder_cfg(dim=Cd, queries=Qn, heads=4, ffn=768, layers=2)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg))
    model = PARQ(cfg).eval()
    W = synth.make_decoder_weights(dcfg, 7901, damped=True)
    Wp = synth.make_ray_pe_weights(Cd, 7902)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("box3d_decoder."):
            src = k[len("box3d_decoder."):].replace("parq_module.decoder.mlp_heads.", "mlp_heads.")
            sd[k] = torch.from_numpy(W[src]).reshape(sd[k].shape)
        else:
            sd[k] = torch.from_numpy(Wp[k[len("add_ray_pe."):]])
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    dec = model.box3d_decoder
    dec.attention_mode = "split"
    dec._expect = ("split", 0)
    model.batch_invariant = True
    assert dec.batch_invariant is True
    cam, T_cp, T_wp, T_wl = synth.make_geometry(7910, 3, V, h, w)
    feat = synth.normal(7911, "feat", (3, V, Cd, h, w), std=0.5)

    def batch(sl):
        return {"all_features": dev(feat[sl]), "camera_feature": Camera(dev(cam[sl])), "T_camera_pseudoCam": Pose(dev(T_cp[sl])),
                "T_world_pseudoCam": Pose(dev(T_wp[sl])), "T_world_local": Pose(dev(T_wl[sl]))}

    def detect(sl):
        with torch.no_grad():
            _, outs = model(batch(sl), 0)
            outs = [{k: o[k].clone() for k in KEYS} for o in outs]
            pred = dec.parse_pred(dict(outs[-1]))
            boxes, mask = raw(pred["obbs_pred"]).clone(), pred["pred_mask"].clone()
        torch.cuda.synchronize()
        assert all(torch.isfinite(o[k]).all() for o in outs for k in KEYS)
        _no_flags(dec)
        return outs, boxes, mask
    all3 = detect(slice(0, 3))
    for i in range(3):
        outs, boxes, mask = detect(slice(i, i + 1))
        assert _diff(all3[0], i, outs) == [], i
        assert torch.equal(all3[2][i:i + 1], mask) and torch.equal(all3[1][i:i + 1], boxes), i
