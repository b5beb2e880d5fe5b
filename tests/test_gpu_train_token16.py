"""GPU tier: training on fp16 / bf16 memory tokens as they are (include/parq_hip.h parq_set_train_token_type).

The reference is always the same module fed ``tokens16.float()``: the fp32 instantiation of every kernel, which the gradient fixtures
pin to the reference's autograd.  A 16-bit value widens to fp32 exactly, so the contract is: the training forward IS the forward on
the upcast (bit for bit, dropout included); in deterministic mode every gradient and the fp32 d_tokens are the upcast step's bits
(this is the test of the two-product fp16 weight-gradient kernel and of every widening load); with the default float atomics the
native step is no further from the upcast step than that step is from itself; and no fp32 copy of the tokens is made."""
import ctypes as C
import functools
import os
import sys
import warnings
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from parq_amd import _lib, synth  # noqa: E402
from parq_amd.decoder import TOKEN_TYPES  # noqa: E402
from gpu_util import make_decoder, scene_args  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d", "sem_cls_prob", "coord_pos")
GRAD_KEYS = (("pred_logits", 10), ("center_unnormalized", 3), ("size_unnormalized", 3), ("ortho6d", 6))
DTYPES = (torch.float16, torch.bfloat16)

# the smallest shapes that reach each path: (dim, heads, ffn, Q, I, B, V, h, w), shared layer weights
CASES = {
    # N = 2070 >= 2048: the batched backward runs kvproj_bwd_split_kernel; B*N = 4140 = 129 x 32 + 12: a ragged last 32-row step
    "split_dw": ((256, 4, 256, 64, 2, 2, 3, 23, 30), True),
    # head dim 256: 16 launch_tn_split_512x256 blocks with channel offsets 0 .. 768; M = 126 rows is ragged
    "wide": ((1024, 4, 256, 32, 2, 1, 2, 7, 9), True),
    # N = 189: the per-iteration backward with gemm_tn
    "generic64": ((256, 4, 256, 64, 3, 2, 3, 7, 9), True),
    # head dim 128
    "generic128": ((512, 4, 256, 32, 2, 1, 2, 7, 9), True),
    # two layers with their own weights: the generic path at N >= 2048
    "unshared": ((256, 4, 256, 64, 2, 2, 3, 23, 30), False),
    # head dim 32 (default mode only: deterministic mode refuses it by design)
    "dh32": ((128, 4, 128, 32, 2, 2, 3, 7, 9), True),
    # `wide` with two layers of their own: the generic path sends a 2048 x 1024 output from 126 rows to the 64 x 64-tile kernel
    "wide_unshared": ((1024, 4, 256, 32, 2, 1, 2, 7, 9), False),
}
ALL = list(CASES)
DET = [c for c in ALL if c != "dh32"]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    (Cd, H, F, Q, I, B, V, h, w), shared = CASES[case]
    seed = 9100 + 10 * ALL.index(case)
    cfg = synth.decoder_cfg(dim=Cd, queries=Q, heads=H, ffn=F, layers=I, share_weights=shared, dropout=0.1)
    W = synth.make_decoder_weights(cfg, seed, damped=True)
    args = scene_args(synth.make_scene(seed + 1, B, V, h, w, Cd, smooth=True))
    g = torch.Generator().manual_seed(seed + 2)
    cots = {k: (torch.randn(I, B, Q, wd, generator=g) * 0.1).cuda() for k, wd in GRAD_KEYS}
    return cfg, W, args, (h, w), cots


def _decoder(case, split8=False):
    """One decoder per case (train mode: dropout 0.1), shared by the tests: packing and workspaces are paid once."""
    return _decoder_cached(case, bool(split8))


@functools.lru_cache(maxsize=None)
def _decoder_cached(case, split8):
    cfg, W, _, _, _ = _inputs(case)
    dec = make_decoder(cfg, W).train()
    if split8:
        dec.attention_mode = "split8"
        dec.train_split8 = True
    return dec


def _eq(a, b):
    """torch.equal, NaN positions compared as a mask."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


def _same(x, y):
    return len(x) == len(y) and all(_eq(a[k], b[k]) for a, b in zip(x, y) for k in KEYS)


def _clone(outs):
    return [{k: v.detach().clone() for k, v in o.items()} for o in outs]


def _step(dec, tokens, case, seed=31):
    """forward_train + backward with the case's fixed cotangents: (outputs, {name: gradient}, d_tokens)."""
    _, _, args, hw, cots = _inputs(case)
    torch.manual_seed(seed)                                   # the dropout seed of the forward
    outs = _clone(dec.forward_train(tokens, *args[1:], feat_hw=hw))
    grads, d_tokens = dec.backward(cots)
    torch.cuda.synchronize()
    assert d_tokens.dtype == torch.float32                    # whatever the tokens' dtype
    g = {k: v.clone() for k, v in grads.items()}
    g["d_tokens"] = d_tokens
    return outs, g


@pytest.fixture
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev)


_REF = {}


def _reference(case, dt, det, split8=False):
    """The upcast step (fp32 instantiations), computed once per (case, dtype, mode) and left unchanged."""
    key = (case, dt, det, split8)
    if key not in _REF:
        assert torch.are_deterministic_algorithms_enabled() == det
        _REF[key] = _step(_decoder(case, split8), _inputs(case)[2][0].to(dt).float(), case)
    return _REF[key]


def _rel(a, b):
    """Relative Frobenius distance."""
    d = (a.double() - b.double()).norm().item()
    n = b.double().norm().item()
    return d / n if n > 0 else d


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ALL)
def test_training_forward_is_the_forward_on_the_upcast(case, dt):
    _, _, args, hw, _ = _inputs(case)
    dec = _decoder(case)
    t16 = args[0].to(dt)
    try:
        for train in (False, True):                            # eval mode with gradients enabled (no dropout), train mode (dropout 0.1)
            dec.train(train)
            got = {}
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                # (eval mode + autograd announces itself once)
                for name, t in (("native", t16), ("upcast", t16.float())):
                    torch.manual_seed(77)
                    o = dec(t, *args[1:], feat_hw=hw)
                    assert o[0]["pred_logits"].requires_grad
                    got[name] = _clone(o)
                    del o
            torch.cuda.synchronize()
            assert all(torch.isfinite(o[k]).all() for o in got["upcast"] for k in KEYS)
            assert _same(got["native"], got["upcast"]), (case, dt, train)
    finally:
        dec.train()


# ------------------------------------------------------------------ 2. deterministic mode: the same bits
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", DET + ["split_dw-split8"])
def test_deterministic_gradients_are_the_upcast_steps_bits(deterministic, case, dt):
    case, split8 = (case.split("-")[0], True) if "-" in case else (case, False)
    want_outs, want = _reference(case, dt, True, split8)
    dec = _decoder(case, split8)
    got_outs, got = _step(dec, _inputs(case)[2][0].to(dt), case)
    assert _same(got_outs, want_outs)
    assert got.keys() == want.keys() and len(got) > 20
    assert all(torch.isfinite(v).all() for v in want.values())
    assert any(v.abs().max() > 0 for k, v in want.items() if "multihead_attn.in_proj" in k)      # the K/V projection gradient is there
    differing = sorted(k for k in want if not torch.equal(got[k], want[k]))
    assert differing == [], (case, dt, differing)


# ------------------------------------------------------------------ 3. default mode (float atomics): within the reference's own noise
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ALL)
def test_default_mode_gradients_are_within_the_upcast_steps_own_noise(case, dt):
    """Per gradient tensor: the relative Frobenius distance native <-> upcast must not exceed the run-to-run noise of the upcast step
    itself — the largest distance among three repeats on the same inputs, times 4 (three repeats underestimate the tail) — capped at
    8e-6, the documented gradient bound, so that a noisy reference cannot hide a real error."""
    assert not torch.are_deterministic_algorithms_enabled()
    dec = _decoder(case)
    t16 = _inputs(case)[2][0].to(dt)
    reps = [_step(dec, t16.float(), case)[1] for _ in range(3)]
    _, got = _step(dec, t16, case)
    bad = []
    worst = (0.0, 0.0, "")
    for k in reps[0]:
        noise = max(_rel(reps[i][k], reps[j][k]) for i, j in ((0, 1), (0, 2), (1, 2)))
        dist = _rel(got[k], reps[0][k])
        bound = min(4.0 * noise, 8e-6)
        if dist >= worst[0]:
            worst = (dist, noise, k)
        if not dist <= bound:
            bad.append((k, dist, noise))
    print("%s %s: worst native distance %.3e (reference noise %.3e) at %s" % (case, dt, worst[0], worst[1], worst[2]))
    assert bad == [], (case, dt, bad)


# ------------------------------------------------------------------ 4. autograd
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", DET)
def test_autograd_token_gradient_keeps_the_dtype_and_the_bits(deterministic, case, dt):
    _, _, args, hw, cots = _inputs(case)
    dec = _decoder(case)
    res = {}
    for name, t in (("native", args[0].to(dt).requires_grad_()), ("upcast", args[0].to(dt).float().requires_grad_())):
        dec.zero_grad(set_to_none=True)
        torch.manual_seed(41)
        o = dec(t, *args[1:], feat_hw=hw)
        loss = sum((torch.stack([x[k] for x in o]) * cots[k]).sum() for k, _ in GRAD_KEYS)
        loss.backward()
        torch.cuda.synchronize()
        res[name] = (t.grad, {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None})
    g16, g32 = res["native"][0], res["upcast"][0]
    assert g16.dtype == dt and g32.dtype == torch.float32
    assert torch.isfinite(g32).all() and g32.abs().max() > 0
    assert torch.equal(g16, g32.to(dt))
    assert sorted(k for k in res["upcast"][1] if not torch.equal(res["native"][1][k], res["upcast"][1][k])) == []


# ------------------------------------------------------------------ one-off cases
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "bf16"])
def test_the_callers_tensor_is_the_one_read(dt):
    _, _, args, hw, _ = _inputs("generic64")
    dec = _decoder("generic64")
    t16 = args[0].to(dt)
    dec.forward_train(t16, *args[1:], feat_hw=hw)
    kept = dec._train_state[1][0]
    assert kept.dtype == dt and kept.data_ptr() == t16.data_ptr()
    assert dec._train_state[-1] == TOKEN_TYPES[dt]
    # a view that is not contiguous: one 16-bit contiguous copy, as in inference
    wide = torch.zeros(t16.shape[0], t16.shape[1], 2 * t16.shape[2], dtype=dt, device="cuda")
    wide[..., :t16.shape[2]] = t16
    dec.forward_train(wide[..., :t16.shape[2]], *args[1:], feat_hw=hw)
    kept = dec._train_state[1][0]
    assert kept.dtype == dt and kept.is_contiguous() and torch.equal(kept, t16)
    torch.cuda.synchronize()


def test_no_fp32_copy_of_the_tokens_lives_through_the_step():
    """split_dw, bf16, parameters require grad, tokens do not: the peak rise of forward + backward stays under the fp32-token step's
    rise + B*N*C bytes (an upcast held from the forward to the backward would sit 4*B*N*C above it)."""
    _, _, args, hw, cots = _inputs("split_dw")
    dec = _decoder("split_dw")
    t32 = args[0].to(torch.bfloat16).float()
    t16 = t32.to(torch.bfloat16)
    B, N, Cd = t16.shape

    def rise(t):
        def step():
            dec.zero_grad(set_to_none=True)
            o = dec(t, *args[1:], feat_hw=hw)
            sum((torch.stack([x[k] for x in o]) * cots[k]).sum() for k, _ in GRAD_KEYS).backward()
            del o
            torch.cuda.synchronize()
        step()                                                 # steady state: the training workspace of this token type exists
        dec.zero_grad(set_to_none=True)
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        return torch.cuda.max_memory_allocated() - base
    r32, r16 = rise(t32), rise(t16)
    print("peak rise: fp32 tokens %d B, bf16 tokens %d B, B*N*C = %d" % (r32, r16, B * N * Cd))
    assert r16 < r32 + B * N * Cd, (r16, r32, B * N * Cd)


def test_out_of_range_bf16_token_is_rerun_in_fp32_like_its_upcast(deterministic):
    cfg, W, args, hw, _ = _inputs("generic64")
    t16 = args[0].to(torch.bfloat16)
    t16[0, 17, 5] = 61440.0
    d16, d32 = make_decoder(cfg, W).train(), make_decoder(cfg, W).train()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got_outs, got = _step(d16, t16, "generic64")
        want_outs, want = _step(d32, t16.float(), "generic64")
    assert d16.attention_mode == d32.attention_mode == "fp32"
    assert d16._train_state[5] == "fp32" and d16._train_state[-1] == 2 and d16._train_state[1][0].dtype == torch.bfloat16
    assert _same(got_outs, want_outs)
    # the backward read the widened workspace copy of the fp32-mode forward
    assert sorted(k for k in want if not _eq(got[k], want[k])) == []


def test_several_outstanding_forwards_carry_their_token_type(deterministic):
    _, _, args, hw, cots = _inputs("generic64")
    dec = _decoder("generic64").eval()
    try:
        a16 = (args[0] * 1.25).to(torch.bfloat16)
        b32 = args[0].clone()

        def loss_of(o):
            return sum((torch.stack([x[k] for x in o]) * cots[k]).sum() for k, _ in GRAD_KEYS)

        def run(pairs):
            dec.zero_grad(set_to_none=True)
            ts = [t.detach().clone().requires_grad_() for t in pairs]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                total = sum(loss_of(dec(t, *args[1:], feat_hw=hw)) for t in ts)
            total.backward()
            torch.cuda.synchronize()
            return [t.grad for t in ts], {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None}
        (ga,), pa = run([a16])
        (gb,), pb = run([b32])
        (ga2, gb2), pab = run([a16, b32])
        assert ga2.dtype == torch.bfloat16 and gb2.dtype == torch.float32
        assert torch.equal(ga2, ga) and torch.equal(gb2, gb)
        assert sorted(k for k in pab if not torch.equal(pab[k], pa[k] + pb[k])) == []
    finally:
        dec.train()


def test_training_step_of_the_module_hands_the_decoder_bf16_tokens(deterministic):
    from parq_amd import PARQ, Camera, Obb3D, Pose
    B, V, h, w, Cd, Qn = 2, 3, 12, 16, 256, 32
    dcfg = synth.decoder_cfg(dim=Cd, queries=Qn, heads=4, ffn=256, layers=3, dropout=0.1)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25,
                                   MAX_DEPTH=5.25), DECODER=dcfg))
    torch.manual_seed(9301)
    model = PARQ(cfg).cuda().train()
    model.token_dtype = torch.bfloat16
    cam, T_cp, T_wp, T_wl = (torch.from_numpy(a).cuda() for a in synth.make_geometry(9302, B, V, h, w))
    obbs, sym = synth.make_boxes(9303, B, 6, max_box=10)
    feat = torch.from_numpy(synth.normal(9304, "feat", (B, V, Cd, h, w), std=0.5)).cuda().requires_grad_()
    batch = {"all_features": feat, "camera_feature": Camera(cam), "T_camera_pseudoCam": Pose(T_cp), "T_world_pseudoCam": Pose(T_wp),
             "T_world_local": Pose(T_wl), "obbs_padded": Obb3D(torch.from_numpy(obbs).cuda()), "sym": torch.from_numpy(sym).cuda()}

    def step(upcast):
        seen = []

        def pre(mod, a):
            seen.append(a[0].dtype)
            return ((a[0].float(),) + tuple(a[1:])) if upcast else None
        hook = model.box3d_decoder.register_forward_pre_hook(pre)
        try:
            np.random.seed(5)
            torch.manual_seed(5)
            model.zero_grad(set_to_none=True)
            feat.grad = None
            loss = model.training_step(batch, 0)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            hook.remove()
        out = {"loss": loss.detach().clone(), "features.grad": feat.grad.clone()}
        out.update({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        return seen, out, model.box3d_decoder._train_state[1][0].dtype
    seen, got, kept = step(False)
    assert seen == [torch.bfloat16] and kept == torch.bfloat16
    seen, want, kept = step(True)
    assert seen == [torch.bfloat16] and kept == torch.float32
    assert len(want) > 40 and all(torch.isfinite(v).all() for v in want.values())
    assert sorted(k for k in want if not torch.equal(got[k], want[k])) == []


def test_through_the_c_abi_with_both_types_set(deterministic):
    _, _, args, hw, cots = _inputs("generic64")
    dec = _decoder("generic64").eval()
    try:
        lib = _lib.load()
        t16 = args[0].to(torch.float16)
        dec.forward_train(t16.float(), *args[1:], feat_hw=hw)      # packs the weights, settles the mode and deterministic form
        h = dec._handle_in_mode(dec._train_state[5], 0)
        _lib.check(lib.parq_set_dropout(h, 0.0, 0), "parq_set_dropout")
        I, Q = dec.num_layers, dec.num_queries

        def run(tt, tokens):
            assert lib.parq_set_token_type(h, tt) == 0 and lib.parq_set_train_token_type(h, tt) == 0
            dec._tok_set = dec._train_tok_set = tt
            sc, keep, dev = dec._scene(tokens, *args[1:], feat_hw=hw, native16=True)
            ws = torch.empty(lib.parq_train_workspace_bytes(h, sc.B, sc.V, sc.h, sc.w) // 4 + 1, dtype=torch.float32, device=dev)
            outs = dec._alloc_outputs((I, sc.B, Q), dev)
            po = _lib.ParqOutputs(*[_lib.ptr(t) for t in outs])
            _lib.check(lib.parq_forward_train(h, C.byref(sc), _lib.ptr(ws), ws.numel() * 4, C.byref(po), _lib.stream_ptr()), "forward_train")
            pg = _lib.ParqOutputGrads(*[_lib.ptr(cots[k]) for k, _ in GRAD_KEYS])
            arena = torch.empty(lib.parq_grad_arena_bytes(h) // 4, dtype=torch.float32, device=dev)
            d_tok = torch.empty(tokens.shape, dtype=torch.float32, device=dev)
            _lib.check(lib.parq_backward(h, C.byref(sc), _lib.ptr(ws), ws.numel() * 4, C.byref(po), C.byref(pg), _lib.ptr(arena),
                                         _lib.ptr(d_tok), _lib.stream_ptr()), "backward")
            torch.cuda.synchronize()
            del keep
            return outs, arena, d_tok
        want = run(0, t16.float())
        got = run(1, t16)
        # a forgotten training type is an error, not fp16 rows read as floats
        assert lib.parq_set_train_token_type(h, 0) == 0
        dec._train_tok_set = 0
        sc, keep, dev = dec._scene(t16, *args[1:], feat_hw=hw, native16=True)
        po = _lib.ParqOutputs(*[_lib.ptr(t) for t in want[0]])
        assert lib.parq_forward_train(h, C.byref(sc), C.c_void_p(256), 1 << 40, C.byref(po), _lib.stream_ptr()) == 1
        assert b"fp32 tokens" in lib.parq_last_error()
        assert all(torch.equal(a, b) for a, b in zip(got[0], want[0]))
        assert torch.isfinite(want[1]).all() and want[1].abs().max() > 0
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    finally:
        dec.train()
