"""GPU tier: fp16 / bf16 memory tokens taken natively by the inference forward (include/parq_hip.h parq_set_token_type).  A 16-bit
value widens to fp32 exactly and the kernels run the fp32-token arithmetic from the widened rows, so the contract is the strictest one:
the forward on 16-bit tokens IS the forward on their fp32 upcast, bit for bit, in every attention mode, captured or not, through the
range policies, the per-head tiers, the stepping API and InFlight — and no fp32 copy of the tokens is made."""
import ctypes as C
import warnings

import pytest
import torch

from parq_amd import _lib, synth
from parq_amd.inflight import InFlight
import golden_util as G
from gpu_util import make_decoder, scene_args

pytestmark = pytest.mark.gpu

KEYS = ("pred_logits", "center_unnormalized", "size_unnormalized", "ortho6d", "sem_cls_prob", "coord_pos")
DTYPES = (torch.float16, torch.bfloat16)


def _geometry(name):
    # (dim, heads, ffn, queries, iterations, B, V, h, w)
    return {"cfg2": (256, 4, 256, 128, 4, 1, 5, 120, 160),
            "ragged": (256, 4, 256, 64, 3, 2, 3, 7, 9),              # N = 189: not a whole number of 64-key stages
            "shipped": (1024, 4, 1024, 64, 3, 2, 3, 60, 80)}[name]


def _setup(name, seed=7101, mode=None):
    C_, H, F, Q, I, B, V, h, w = _geometry(name)
    cfg = synth.decoder_cfg(dim=C_, queries=Q, heads=H, ffn=F, layers=I)
    W = synth.make_decoder_weights(cfg, seed, damped=True)
    sc = synth.make_scene(seed + 1, B, V, h, w, C_, smooth=True)
    return cfg, W, scene_args(sc), (h, w)


def _dec(cfg, W, mode=None, graph=False, check=None):
    dec = make_decoder(cfg, W)
    if mode:
        dec.attention_mode = mode
    dec.use_graph = graph
    if check:
        dec.range_check = check
    return dec


def _run(dec, tokens, args, hw):
    with torch.no_grad():
        out = [{k: v.clone() for k, v in o.items()} for o in dec(tokens, *args[1:], feat_hw=hw)]
    torch.cuda.synchronize()
    return out


def _eq(a, b):
    """torch.equal, NaN positions compared as a mask."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


def _same(x, y):
    return len(x) == len(y) and all(_eq(a[k], b[k]) for a, b in zip(x, y) for k in KEYS)


def _replays(dec):
    return sum(e.replays for e in dec._ws.values())


@pytest.mark.parametrize("name", ["cfg2", "ragged", "shipped"])
@pytest.mark.parametrize("mode", ["split8", "split", "fp32", "fp16", "bf16"])
def test_16_bit_tokens_give_the_forward_on_their_fp32_upcast(name, mode):
    cfg, W, args, hw = _setup(name)
    dec = _dec(cfg, W, mode, check="off")
    for dt in DTYPES:
        t16 = args[0].to(dt)
        want = _run(dec, t16.float(), args, hw)
        got = _run(dec, t16, args, hw)
        assert dec.attention_mode == mode
        assert _same(got, want), (name, mode, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_captured_and_replayed_16_bit_forwards(dt):
    cfg, W, args, hw = _setup("ragged", seed=7201)
    t16 = args[0].to(dt)
    want = _run(_dec(cfg, W), t16.float(), args, hw)
    dec = _dec(cfg, W, graph=True)
    runs = [_run(dec, t16, args, hw) for _ in range(3)]          # launch by launch, captured + replayed, replayed
    assert _replays(dec) == 2
    assert all(_same(r, want) for r in runs)


def test_alternating_token_types_never_replay_across_types():
    cfg, W, args, hw = _setup("ragged", seed=7301)
    types = (torch.float32, torch.bfloat16, torch.float16)
    ref = _dec(cfg, W)
    want = {dt: _run(ref, args[0].to(dt), args, hw) for dt in types}
    dec = _dec(cfg, W, graph=True)
    for rep in range(2):
        for dt in types:
            assert _same(_run(dec, args[0].to(dt), args, hw), want[dt]), (rep, dt)
    assert _replays(dec) == 0, "a key that never repeats back to back is never captured"
    for dt in types:                                            # each type: captured and replayed under its own key
        before = _replays(dec)
        for _ in range(3):
            assert _same(_run(dec, args[0].to(dt), args, hw), want[dt]), dt
        assert _replays(dec) == before + 2
    entry = next(reversed(dec._ws.values()))
    assert [k[-1] for k in entry.graphs] == [1]                 # the last type's (fp16): a capture retires the graphs of other keys


def test_capture_and_replay_through_the_c_abi_check_the_token_type():
    cfg, W, args, hw = _setup("ragged", seed=7401)
    dec = _dec(cfg, W, check="off")
    t16 = args[0].to(torch.bfloat16)
    want = _run(dec, t16, args, hw)
    lib, h = _lib.load(), dec._handle()
    sc, keep, dev_ = dec._scene(t16, *args[1:], feat_hw=hw, native16=True)
    assert keep[0].dtype == torch.bfloat16
    dec._token_type(h, 0)
    ws = dec._workspace(sc.B, sc.V, sc.h, sc.w, dev_)
    g = C.c_void_p()
    _lib.check(lib.parq_forward_capture(h, sc.B, sc.V, sc.h, sc.w, _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr(), C.byref(g)), "capture")
    outs = dec._alloc_outputs((dec.num_layers, sc.B, dec.num_queries), dev_)
    po = _lib.ParqOutputs(*[_lib.ptr(t) for t in outs])
    assert lib.parq_set_token_type(h, 2) == 0
    dec._tok_set = 2
    assert lib.parq_forward_replay(h, g, C.byref(sc), _lib.ptr(ws), ws.numel() * 4, C.byref(po), _lib.stream_ptr()) == 3
    assert b"token type" in lib.parq_last_error()
    assert lib.parq_set_token_type(h, 7) == 1
    # recorded under type 2: the replay is the forward
    assert lib.parq_graph_destroy(g) == 0
    g = C.c_void_p()
    _lib.check(lib.parq_forward_capture(h, sc.B, sc.V, sc.h, sc.w, _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr(), C.byref(g)), "capture")
    _lib.check(lib.parq_forward_replay(h, g, C.byref(sc), _lib.ptr(ws), ws.numel() * 4, C.byref(po), _lib.stream_ptr()), "replay")
    torch.cuda.synchronize()
    for i, key in enumerate(KEYS):
        for k in range(dec.num_layers):
            assert torch.equal(outs[i][k], want[k][key]), (key, k)
    assert lib.parq_graph_destroy(g) == 0


@pytest.mark.parametrize("dt,value", [(torch.bfloat16, 61440.0), (torch.float16, 65504.0), (torch.float16, float("inf"))])
@pytest.mark.parametrize("check", ["sync", "lazy", "off"])
def test_out_of_range_16_bit_tokens_meet_the_policy_like_their_upcast(dt, value, check):
    cfg, W, args, hw = _setup("ragged", seed=7501)
    t16 = args[0].to(dt)
    t16[0, 17, 5] = value
    d16, d32 = _dec(cfg, W, check=check), _dec(cfg, W, check=check)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = _run(d16, t16, args, hw)
        want = _run(d32, t16.float(), args, hw)
    assert _same(got, want)
    assert d16.attention_mode == d32.attention_mode
    if check == "sync":
        assert d16.attention_mode == "fp32"
    else:
        assert d16.fp16_range_exceeded() == d32.fp16_range_exceeded()
        assert d16.attention_min_row_sum() == d32.attention_min_row_sum()


def test_peaked_attention_tiers_follow_the_upcast():
    case, _ = G.load("g15_cfg5_shape")
    cfg, W, sc = G.inputs(case)
    W = dict(W)
    wq = "parq_module.decoder.layers.0.multihead_attn.in_proj_weight"
    w = W[wq].copy()
    w[:w.shape[1]] *= 4.0
    W[wq] = w
    args = scene_args(sc)
    t16 = args[0].to(torch.bfloat16)
    d16, d32 = make_decoder(cfg, W), make_decoder(cfg, W)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = _run(d16, t16, args, None)
        want = _run(d32, t16.float(), args, None)
    assert d16.safe_heads == d32.safe_heads
    assert _same(got, want)


def test_inflight_16_bit_scenes_equal_the_serial_forwards():
    cfg, W, args, hw = _setup("ragged", seed=7601)
    scenes = [(args[0] * (1.0 + 0.25 * i)).to(dt) for i, dt in enumerate((torch.bfloat16, torch.float16, torch.bfloat16))]
    ref = _dec(cfg, W)
    want = [_run(ref, t, args, hw) for t in scenes]
    dec = _dec(cfg, W, graph=True)
    fl = InFlight(dec, depth=2)
    with torch.no_grad():
        tickets = [fl.submit(t, *args[1:], feat_hw=hw) for t in scenes]
        got = [[{k: v.clone() for k, v in o.items()} for o in tk.result()] for tk in tickets]
    fl.drain()
    assert all(_same(g, w) for g, w in zip(got, want))


def test_stepping_api_takes_16_bit_tokens():
    cfg, W, args, hw = _setup("ragged", seed=7701)
    dec = _dec(cfg, W)
    t16 = args[0].to(torch.bfloat16)
    want = _run(dec, t16.float(), args, hw)
    with torch.no_grad():
        dec.prepare(t16, *args[1:], feat_hw=hw)
        steps = [{k: v.clone() for k, v in dec.iterate(k)[0].items()} for k in range(dec.num_layers)]
    torch.cuda.synchronize()
    assert _same(steps, want)


def test_no_fp32_copy_of_16_bit_tokens():
    cfg, W, args, hw = _setup("cfg2", seed=7801)
    t16 = args[0].to(torch.bfloat16)
    B, N, Cd = t16.shape
    dec = _dec(cfg, W, graph=True)
    _run(dec, t16, args, hw)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        out = dec(t16, *args[1:], feat_hw=hw)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise < B * N * Cd, (rise, B * N * Cd)
    del out
    lib, h = _lib.load(), dec._handle()
    sizes = {}
    for tt in (0, 2):
        dec._token_type(h, tt)
        sizes[tt] = lib.parq_workspace_bytes(h, B, 5, 120, 160)
    assert 0 < sizes[2] <= sizes[0], sizes


def test_training_with_16_bit_tokens_is_unchanged():
    cfg, W, args, hw = _setup("ragged", seed=7901)
    dec = make_decoder(cfg, W)
    t16 = args[0].to(torch.bfloat16).requires_grad_()
    t32 = t16.detach().float().requires_grad_()
    outs = []
    for t in (t16, t32):
        o = dec(t, *args[1:], feat_hw=hw)
        loss = sum((o[k]["center_unnormalized"] * (k + 1)).sum() + o[k]["pred_logits"].square().mean() for k in range(len(o)))
        loss.backward()
        outs.append([{k: v.detach().clone() for k, v in x.items()} for x in o])
    torch.cuda.synchronize()
    assert _same(outs[0], outs[1])
    assert t16.grad.dtype == torch.bfloat16
    # (the chain backward accumulates with float atomics: the two gradients agree to that order, then to bf16 rounding)
    assert torch.allclose(t16.grad.float(), t32.grad, rtol=1e-2, atol=1e-6)


def _ray_pe(Cd, S, seed):
    from parq_amd import AddRayPE
    Wp = synth.make_ray_pe_weights(Cd, seed, num_samples=S)
    pe = AddRayPE(Cd, synth.DEFAULT_SCALE, S, 0.25, 5.25)
    pe.load_state_dict({k: torch.from_numpy(v) for k, v in Wp.items()}, strict=True)
    return pe.cuda().eval(), Wp


@pytest.mark.parametrize("Cd,S", [(256, 64), (128, 64), (256, 128)])          # the one-pass kernel, and the two-GEMM path twice
def test_ray_pe_writes_16_bit_tokens_rounded_like_torch(Cd, S):
    pe, _ = _ray_pe(Cd, S, 8101)
    B, V, h, w = 2, 3, 11, 23                                                  # a ragged last tile
    cam, T_cp, T_wp, T_wl = (torch.from_numpy(a).cuda() for a in synth.make_geometry(8102, B, V, h, w))
    feat = torch.from_numpy(synth.normal(8103, "feat", (B, V, Cd, h, w), std=3.0)).cuda()
    feat[0, 1, 5, 2, 3] = 70000.0                                              # past fp16's range: +inf in fp16, finite in bf16
    feat[1, 0, 7, 4, 4] = float("nan")
    with torch.no_grad():
        want32 = pe.tokens(feat, cam, T_cp, T_wp, T_wl)
        for dt in DTYPES:
            got = pe.tokens(feat, cam, T_cp, T_wp, T_wl, dtype=dt)
            assert got.dtype == dt and got.shape == want32.shape
            assert _eq(got.float(), want32.to(dt).float()), (Cd, S, dt)
            assert _eq(pe.tokens(feat, cam, T_cp, T_wp, T_wl).to(dt).float(), want32.to(dt).float())     # fp32 calls unchanged after it
    # with a graph: the fp32 autograd node, then the conversion
    feat.requires_grad_()
    t = pe.tokens(feat, cam, T_cp, T_wp, T_wl, dtype=torch.bfloat16)
    assert t.dtype == torch.bfloat16 and t.requires_grad
    assert _eq(t.detach().float(), want32.to(torch.bfloat16).float())


def test_parq_module_with_bf16_tokens_feeds_the_decoder_16_bit_tokens():
    from types import SimpleNamespace as NS
    from parq_amd import PARQ, Camera, Pose
    B, V, h, w, Cd, Qn = 2, 3, 12, 16, 256, 32
    dcfg = synth.decoder_cfg(dim=Cd, queries=Qn, heads=4, ffn=256, layers=3)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25,
                                   MAX_DEPTH=5.25), DECODER=dcfg))
    model = PARQ(cfg).eval()
    W = synth.make_decoder_weights(dcfg, 8201, damped=True)
    Wp = synth.make_ray_pe_weights(Cd, 8202)
    sd = model.state_dict()
    for k in sd:
        if k.startswith("box3d_decoder."):
            sd[k] = torch.from_numpy(W[k[len("box3d_decoder."):].replace("parq_module.decoder.mlp_heads.", "mlp_heads.")]).reshape(sd[k].shape)
        else:
            sd[k] = torch.from_numpy(Wp[k[len("add_ray_pe."):]])
    model.load_state_dict(sd, strict=True)
    model = model.cuda()
    model.box3d_decoder.use_graph = False
    cam, T_cp, T_wp, T_wl = (torch.from_numpy(a).cuda() for a in synth.make_geometry(8203, B, V, h, w))
    feat = torch.from_numpy(synth.normal(8204, "feat", (B, V, Cd, h, w), std=0.5)).cuda()
    batch = {"all_features": feat, "camera_feature": Camera(cam), "T_camera_pseudoCam": Pose(T_cp),
             "T_world_pseudoCam": Pose(T_wp), "T_world_local": Pose(T_wl)}
    model.token_dtype = torch.bfloat16
    seen = []
    hook = model.box3d_decoder.register_forward_pre_hook(lambda mod, args: seen.append(args[0].dtype))
    with torch.no_grad():
        _, got = model(batch, 0)
        got = [{k: v.clone() for k, v in o.items()} for o in got]
        hook.remove()
        tok = model.add_ray_pe.tokens(feat, Camera(cam), Pose(T_cp), Pose(T_wp), Pose(T_wl)).to(torch.bfloat16)
        want = _run(model.box3d_decoder, tok, (tok, Camera(cam), Pose(T_cp), Pose(T_wp), Pose(T_wl)), (h, w))
    assert seen == [torch.bfloat16]
    assert _same(got, want)


def test_fp16_and_bf16_share_the_widened_workspace_of_mode_fp32():
    cfg, W, args, hw = _setup("ragged", seed=8301)
    dec = _dec(cfg, W, "fp32")
    ref = _dec(cfg, W, "fp32")
    for dt in (torch.bfloat16, torch.float16, torch.bfloat16, torch.float32):
        assert _same(_run(dec, args[0].to(dt), args, hw), _run(ref, args[0].to(dt).float(), args, hw)), dt
    assert sorted(len(k) for k in dec._ws) == [6, 7]          # one workspace for fp32 tokens, one (with the widened copy) for both 16-bit types
