"""GPU tier: which kernel's numbers reach the caller, across the states of the module — attention mode x range_check policy x captured
graph x one-at-a-time calls or forwards in flight (parq_amd.InFlight).  The kernels themselves are pinned elsewhere against float64; here
the decision layer is: under the default policy ("sync") no forward hands out NaN, whether its check runs inside the call or is deferred
to Ticket.result(), and whatever other forwards in flight did to the module meanwhile.

Scenes (fixture g15_cfg5_shape: d = 256, head dim 64, mode "split8" with its peakedness guard live):
  * diffuse: the fixture as captured;
  * peaked: tokens x 4 — rows that two or three keys carry, all four heads trip the guard;
  * out of range: tokens x 2e4 — token elements beyond the fp16 range.
Serial expectations (fresh modules, same scene): a diffuse scene gives the output of the mode the module is in; a peaked scene in mode
"split8" gives mode "split"'s output bit for bit (all heads safe IS mode "split"); an out-of-range scene in an fp16-operand mode gives
mode "fp32"'s output bit for bit.  The expectations themselves are checked against the float64 oracle."""
import warnings

import numpy as np
import pytest
import torch

from parq_amd import InFlight, synth
from oracle import parq_oracle as O
import golden_util as G
from gpu_util import make_decoder, rel_err, scene_args

pytestmark = pytest.mark.gpu

FP16_MODES = ("split", "split8", "fp16")
_CACHE = {}


def _setup():
    if "setup" not in _CACHE:
        case, _ = G.load("g15_cfg5_shape")
        cfg, W, sc = G.inputs(case)
        scenes = {"diffuse": sc, "peaked": dict(sc), "oor": dict(sc)}
        scenes["peaked"]["tokens"] = (sc["tokens"] * np.float32(4.0)).astype(np.float32)
        scenes["oor"]["tokens"] = (sc["tokens"] * np.float32(2e4)).astype(np.float32)
        args = {k: scene_args(v) for k, v in scenes.items()}
        _CACHE["setup"] = (cfg, W, scenes, args)
    return _CACHE["setup"]


def _clone(outs):
    return [{k: v.clone() for k, v in o.items()} for o in outs]


def _decoder(mode=None, policy="sync", graph=True):
    cfg, W, _, _ = _setup()
    dec = make_decoder(cfg, W).eval()
    if mode is not None:
        dec.attention_mode = mode
    dec.range_check = policy
    dec.use_graph = graph
    return dec


def _expected(scene, mode, policy="sync"):
    """Output of a fresh module in `mode` on `scene` (its first forward: no graph, no earlier state)."""
    key = (scene, mode, policy)
    if key not in _CACHE:
        dec = _decoder(mode, policy)
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _CACHE[key] = _clone(dec(*_setup()[3][scene]))
        torch.cuda.synchronize()
        assert dec.attention_mode == mode and dec.safe_heads == 0, "the expectation itself must not have moved"
    return _CACHE[key]


def _equal(a, b):
    """Bit-identical outputs (NaN where the other has NaN)."""
    return all(torch.equal(torch.nan_to_num(x[k], nan=7.25), torch.nan_to_num(y[k], nan=7.25)) and
               torch.equal(torch.isnan(x[k]), torch.isnan(y[k])) for x, y in zip(a, b) for k in x)


def _finite(outs):
    return all(bool(torch.isfinite(v).all()) for o in outs for v in o.values())


def _assert_one_of(got, scene, modes, what):
    assert _finite(got), (what, "NaN handed out")
    assert any(_equal(got, _expected(scene, m)) for m in modes), (what, "equals none of the serial outputs of", modes)


def _serial_state(mode, scene):
    """The mode whose numbers a serial call under "sync" returns for `scene` in a module currently computing in `mode`, and the state
    after it."""
    if scene == "peaked" and mode == "split8":
        return "split"                      # the four flagged heads move: a module whose heads are all safe runs mode "split"
    if scene == "oor" and mode in FP16_MODES:
        return "fp32"
    return mode


# ---------------------------------------------------------------------------------------------------------- the expectations vs float64

def _oracle_error(scene, mode):
    """Worst teacher-forced error of the expectation against the float64 oracle (reference points forced to the module's own per-iteration
    outputs, as tests/test_gpu_range.py::_decoder_errors does); size_unnormalized only where the arg-max class is not within rounding of
    flipping."""
    cfg, W, scenes, _ = _setup()
    sc = scenes[scene]
    outs = [{k: v.cpu().numpy() for k, v in o.items()} for o in _expected(scene, mode)]
    od = O.OracleDecoder(cfg, W, synth.SCANNET_MEAN_SIZES, dtype=torch.float64)
    forced = [O.normalize(torch.from_numpy(o["coord_pos"]).double(), cfg.TRANSFORMER.SCALE) for o in outs]
    with torch.no_grad():
        want = od.forward(sc["tokens"], sc["camera"], sc["T_camera_pseudoCam"], sc["T_world_pseudoCam"], sc["T_world_local"],
                          forced_refs=forced)
    worst = 0.0
    for a, b in zip(outs, want):
        top2 = b["sem_cls_prob"].topk(2, -1).values
        ok = ((top2[..., 0] - top2[..., 1]) > 1e-3).numpy()
        for key in a:
            x, y = a[key], b[key].numpy()
            if key == "size_unnormalized":
                x, y = x[ok], y[ok]
            worst = max(worst, rel_err(x, y) if np.isfinite(x).all() else float("inf"))
    return worst


# 1e-4: tests/test_gpu_range.py's bound for the whole decoder against float64 (measured 2.5e-5 diffuse, 5.7e-5 peaked, 12 iterations).
# Out of range (tokens x 2e4) every cross-attention row is one-hot and fp32 rounding of the scores decides near-ties between keys — the
# limit of the reference's own arithmetic (tests/test_gpu_range.py); 1e-2 still separates fp32-class numbers (measured 5.7e-3) from wrong ones.
@pytest.mark.parametrize("scene,mode,bound", [("diffuse", "split8", 1e-4), ("diffuse", "split", 1e-4), ("peaked", "split", 1e-4),
                                              ("oor", "fp32", 1e-2)])
def test_serial_expectations_against_float64(scene, mode, bound):
    e = _oracle_error(scene, mode)
    print("\n%s scene, mode %s: teacher-forced vs float64 %.2e" % (scene, mode, e))
    assert e < bound, e


# ------------------------------------------------------------------------------------ deferred checks of several forwards in flight

def _inflight_module():
    """A default module (mode "split8", policy "sync") past its first forward, which every policy checks synchronously."""
    dec = _decoder()
    with torch.no_grad():
        dec(*_setup()[3]["diffuse"])
    torch.cuda.synchronize()
    return dec


def _submit_all(dec, depth, scenes):
    args = _setup()[3]
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        runner = InFlight(dec, depth=depth)
        tickets = [runner.submit(*args[s]) for s in scenes]
        got = [_clone(t.result()) for t in tickets]
    torch.cuda.synchronize()
    return got


def test_two_peaked_scenes_in_flight_both_settle_to_mode_split():
    dec = _inflight_module()
    got = _submit_all(dec, 2, ["peaked", "peaked"])
    for i, g in enumerate(got):
        assert _finite(g), (i, "NaN handed out")
        assert _equal(g, _expected("peaked", "split")), i
    assert dec.safe_heads == 0b1111


def test_two_out_of_range_scenes_in_flight_both_settle_to_mode_fp32():
    dec = _inflight_module()
    got = _submit_all(dec, 2, ["oor", "oor"])
    for i, g in enumerate(got):
        assert _finite(g), (i, "NaN handed out")
        assert _equal(g, _expected("oor", "fp32")), i
    assert dec.attention_mode == "fp32"


def test_peaked_then_out_of_range_scene_in_flight_each_gets_its_own_fallback():
    dec = _inflight_module()
    got = _submit_all(dec, 2, ["peaked", "oor"])
    assert _finite(got[0]) and _equal(got[0], _expected("peaked", "split"))
    assert _finite(got[1]) and _equal(got[1], _expected("oor", "fp32"))
    assert dec.attention_mode == "fp32"


def test_a_later_submit_does_not_take_the_flag_of_a_pending_ticket():
    """The documented pattern: A.result(), then submit(C) while B is pending.  C's submit polls the module's pinned words; B's word
    belongs to B's deferred check and must still be there when B.result() looks."""
    dec = _inflight_module()
    args = _setup()[3]
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        runner = InFlight(dec, depth=2)
        ta = runner.submit(*args["diffuse"])
        tb = runner.submit(*args["peaked"])
        a = _clone(ta.result())
        torch.cuda.synchronize()                         # B has surely raised its flag into the pinned word by now
        tc = runner.submit(*args["diffuse"])
        b = _clone(tb.result())
        c = _clone(tc.result())
    torch.cuda.synchronize()
    assert _finite(a) and _equal(a, _expected("diffuse", "split8"))
    assert _finite(b), "B's flag was taken by C's submit: NaN handed out"
    assert _equal(b, _expected("peaked", "split"))
    _assert_one_of(c, "diffuse", ("split8", "split"), "C")     # serial semantics allow C either tier
    assert dec.safe_heads == 0b1111


@pytest.mark.parametrize("depth", [2, 3])
def test_more_tickets_than_streams(depth):
    """Four submits before any result(): at depth 2 (and 3) two forwards share a stream, a workspace and its mirror slot."""
    dec = _inflight_module()
    seq = ["diffuse", "peaked", "diffuse", "peaked"]
    got = _submit_all(dec, depth, seq)
    for i, (s, g) in enumerate(zip(seq, got)):
        if s == "peaked":
            assert _finite(g), (i, "NaN handed out")
            assert _equal(g, _expected("peaked", "split")), i
        else:
            _assert_one_of(g, "diffuse", ("split8", "split"), i)
    assert _equal(got[0], _expected("diffuse", "split8"))     # nothing can have moved the heads before the first forward ran
    assert dec.safe_heads == 0b1111


# --------------------------------------------------------------------------------------------------------------------- the state walk

WALK = ["diffuse", "peaked", "diffuse", "peaked", "diffuse"]     # the second diffuse call is the first to replay a captured graph
OOR_LEG = ["diffuse", "oor", "diffuse"]


def _walk_cases():
    out = []
    for mode in ("split8", "split", "fp16", "fp32"):
        for policy in ("sync", "lazy", "off"):
            if mode == "fp32" and policy != "sync":
                continue                    # the exact-fp32 kernels raise no flag: every policy is the same code path as "sync"
            for inflight in (False, True):
                if inflight and policy == "lazy":
                    continue                # "lazy" is never deferred: InFlight changes nothing there (test_lazy_submit_does_not_wait)
                for graph in (True, False):
                    out.append(pytest.param(mode, policy, graph, inflight,
                                            id="%s-%s-%s-%s" % (mode, policy, "graph" if graph else "nograph", "inflight" if inflight else "serial")))
    return out


def _run_sequence(dec, seq, inflight, reports=None):
    """Outputs of `seq` on `dec`; serial calls append (attention_too_peaked(), fp16_range_exceeded()) of each call to `reports`."""
    args = _setup()[3]
    got = []
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if inflight:
            runner = InFlight(dec, depth=2)
            tickets = [runner.submit(*args[s]) for s in seq]
            got = [_clone(t.result()) for t in tickets]
        else:
            for s in seq:
                got.append(_clone(dec(*args[s])))
                torch.cuda.synchronize()        # (serial: the next call's poll of the pinned words sees what this one raised)
                if reports is not None:
                    reports.append((dec.attention_too_peaked(), dec.fp16_range_exceeded()))
    torch.cuda.synchronize()
    return got


def _nan_suffix(outs):
    """Index of the first iteration whose outputs (but the input reference points) are all NaN, every later one NaN too and every
    earlier one finite; None if the structure is anything else."""
    first = None
    for i, o in enumerate(outs):
        nan = all(bool(torch.isnan(v).all()) for k, v in o.items() if k != "coord_pos")
        fin = all(bool(torch.isfinite(v).all()) for v in o.values())
        if first is None and nan:
            first = i
        elif first is None and not fin:
            return None
        elif first is not None and not nan:
            return None
    return first


def _check_walk(mode, policy, seq, got, inflight):
    state = mode
    for i, (s, g) in enumerate(zip(seq, got)):
        what = (i, s, state)
        if policy == "sync":
            after = _serial_state(state, s)
            if not inflight:
                assert _finite(g), (what, "NaN handed out")
                assert _equal(g, _expected(s, after)), what
            elif s == "diffuse":
                # in flight a diffuse forward may run before or after an earlier ticket's check moved the module
                seen = {mode}
                for x in seq[:i]:
                    seen |= {_serial_state(m, x) for m in seen}
                _assert_one_of(g, s, sorted(seen), what)
            else:
                assert _finite(g), (what, "NaN handed out")
                assert _equal(g, _expected(s, after)), what
            state = after
        elif policy == "lazy":
            flagged = _serial_state(state, s) != state
            if flagged:
                first = _nan_suffix(g)
                assert first is not None, (what, "finite numbers from outside the error model")
                assert all(_equal([a], [b]) for a, b in zip(g[:first], _expected(s, state, "off")[:first])), what
                state = _serial_state(state, s)           # the NEXT call polls the word and switches
            else:
                assert _finite(g) and _equal(g, _expected(s, state)), what
        else:                                             # "off": no poisoning, no tier change, the report on request
            assert _equal(g, _expected(s, mode, "off")), what
            if s != "oor":
                assert _finite(g), what
    if policy == "off":
        assert state == mode


@pytest.mark.parametrize("mode,policy,graph,inflight", _walk_cases())
def test_policy_state_walk(mode, policy, graph, inflight):
    dec = _decoder(mode, policy, graph)
    reports = []
    got = _run_sequence(dec, WALK, inflight, reports)
    _check_walk(mode, policy, WALK, got, inflight)
    if policy == "off":
        assert dec.safe_heads == 0 and dec.attention_mode == mode
        if mode == "split8" and not inflight:
            assert [r[0] for r in reports] == [s == "peaked" for s in WALK], reports     # the report names the peaked calls
    if policy == "sync" and mode == "split8":
        assert dec.safe_heads == 0b1111
    key = (mode, policy, inflight)
    other = _CACHE.setdefault(("walk",) + key, {})
    other[graph] = got
    if len(other) == 2:                                   # graph on and off: the same numbers, call by call
        assert all(_equal(a, b) for a, b in zip(other[True], other[False]))


@pytest.mark.parametrize("policy", ["sync", "lazy", "off"])
@pytest.mark.parametrize("mode", ["split8", "split"])
def test_out_of_range_leg(mode, policy):
    dec = _decoder(mode, policy)
    reports = []
    got = _run_sequence(dec, OOR_LEG, False, reports)
    _check_walk(mode, policy, OOR_LEG, got, False)
    if policy == "off":
        assert [r[1] for r in reports] == [s == "oor" for s in OOR_LEG], reports
        assert dec.attention_mode == mode
    else:
        assert dec.attention_mode == "fp32"
    if policy == "sync":
        got = _run_sequence(_decoder(mode, policy), OOR_LEG, True)
        _check_walk(mode, policy, OOR_LEG, got, True)


def test_lazy_submit_does_not_wait():
    """"lazy" under InFlight: submit() enqueues and returns — the peaked forward's flag is not looked at until a later call polls."""
    dec = _inflight_module()
    dec.range_check = "lazy"
    args = _setup()[3]
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        runner = InFlight(dec, depth=2)
        t = runner.submit(*args["peaked"])
        assert dec.safe_heads == 0 and not t._settle
        out = _clone(t.result())
    torch.cuda.synchronize()
    assert _nan_suffix(out) is not None and not t.valid()


# ----------------------------------------------------------------------------------------------------------------- the PARQ wrapper

def test_inflight_over_the_parq_module_with_losses_and_a_peaked_middle_snippet():
    """InFlight over parq_amd.PARQ with ground truth in the batch (the set loss is computed inside the call) and the middle snippet's
    cross-attention peaked: outputs and losses from result() equal those of one-at-a-time calls — the losses are those of the settled
    (re-run) outputs, not of the poisoned first attempt."""
    from types import SimpleNamespace as NS
    from parq_amd import PARQ, Camera, Obb3D, Pose
    from gpu_util import dev
    B, V, h, w, Cd, Qn, I = 1, 4, 48, 64, 256, 64, 3
    dcfg = synth.decoder_cfg(dim=Cd, queries=Qn, heads=4, ffn=768, layers=I)
    pcfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=Cd, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                       DECODER=dcfg))
    W = synth.make_decoder_weights(dcfg, 811)
    Wp = synth.make_ray_pe_weights(Cd, 812)

    def build():
        model = PARQ(pcfg).eval()
        sd = model.state_dict()
        for k in sd:
            if k.startswith("box3d_decoder."):
                src = k[len("box3d_decoder."):].replace("parq_module.decoder.mlp_heads.", "mlp_heads.")
                sd[k] = torch.from_numpy(W[src]).reshape(sd[k].shape)
            else:
                sd[k] = torch.from_numpy(Wp[k[len("add_ray_pe."):]])
        model.load_state_dict(sd, strict=True)
        return model.cuda()

    def snippet(seed, gain):
        cam, T_cp, T_wp, T_wl = synth.make_geometry(seed, B, V, h, w)
        feat = synth.normal(seed + 1, "feat", (B, V, Cd, h, w), std=1.0) * np.float32(gain)
        obbs, sym = synth.make_boxes(seed + 2, B, 5, max_box=8)
        return {"all_features": dev(feat), "camera_feature": Camera(dev(cam)), "T_camera_pseudoCam": Pose(dev(T_cp)),
                "T_world_pseudoCam": Pose(dev(T_wp)), "T_world_local": Pose(dev(T_wl)), "obbs_padded": Obb3D(dev(obbs)), "sym": dev(sym)}
    snippets = [snippet(820, 1.0), snippet(830, 6.0), snippet(840, 1.0)]

    def losses_of(losses):
        return {k: v.detach().double().cpu() for k, v in losses.items() if torch.is_tensor(v)}

    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = build()
        want = []
        for b in snippets:
            losses, outs = model(dict(b), 0)
            want.append((losses_of(losses), _clone(outs)))
        torch.cuda.synchronize()
        assert model.box3d_decoder.safe_heads == 0b1111, "the x 6 snippet is meant to trip the guard on every head"
        model = build()
        runner = InFlight(model, depth=2)
        tickets = [runner.submit(dict(b), 0) for b in snippets]
        got = []
        for t in tickets:
            losses, outs = t.result()
            got.append((losses_of(losses), _clone(outs)))
        torch.cuda.synchronize()
    for i, ((lw, ow), (lg, og)) in enumerate(zip(want, got)):
        assert _finite(og), (i, "NaN handed out")
        assert _equal(og, ow), i
        assert lw.keys() == lg.keys() and "total_loss" in lg, i
        for k in lw:
            assert torch.isfinite(lg[k]).all(), (i, k)
            torch.testing.assert_close(lg[k], lw[k], rtol=1e-6, atol=0, msg=lambda m, i=i, k=k: "%s %s: %s" % (i, k, m))
