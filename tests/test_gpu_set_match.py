"""GPU tier of the device matcher: parq_set_match (parq_amd/csrc/setmatch.hip) against its NumPy statements (tests/set_match_cases.py) —
the cost against a float64 evaluation, everything behind the cost bit for bit on the kernel's own cost — and PARQDecoder.loss with
match_on_device against the host matcher: same pairs, same step, and no dependence on np.random where the cap binds.

Cost tolerance: 32 * 2^-24 * max(1, |m64|): a softmax of at most 10 classes (expf within two ulp, a 10-term sum, one division) scaled
by cost_class = 2, plus the two roundings of the products and the difference.  Measured: profiles/set_match_errors.txt."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
from make_golden import LOSS_CASE, loss_case_inputs  # noqa: E402  (inputs regenerated from the seed: data only)
from parq_amd import Obb3D, Pose, _lib, synth  # noqa: E402
from parq_amd.loss import HungarianMatcherModified, parse_target  # noqa: E402
from gpu_util import dev, lib, make_decoder, sptr  # noqa: E402
from tail_oracles import set_loss_oracle  # noqa: E402
from test_gpu_set_loss_kernel import compare, rot_rows_left_out  # noqa: E402

import set_match_cases as M  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, PATTERN = 64, 0x5A5A5A5A
TERMS = ("center_loss", "size_loss", "rot_loss", "cat_loss", "total_loss")
CASES = [(s, v) for s in M.SHAPES for v in M.VARIANTS]
OUT_KEYS = ("row_to_col", "pairs", "pair_coef", "row_weight", "stats")


def run_match(c, seed, step, logits=None):
    """One parq_set_match call on a case: the outputs as NumPy arrays plus cost_out / near_out.  Every output has a guard behind it,
    which must come back untouched; columns the entry does not write keep the fill value."""
    I, B, Q, ncls, nmax = c["I"], c["B"], c["Q"], c["ncls"], c["nmax"]
    S, P = I * B, I * B * Q
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    lg, cp, tc, tl, tn = cu(c["logits"] if logits is None else logits), cu(c["coord"]), cu(c["t_center"]), cu(c["t_label"]), cu(c["t_count"])
    l = lib()
    need = l.parq_set_match_workspace_bytes(I, B, Q, nmax)
    assert need > 0 and need % 16 == 0
    buf = lambda n, dt=torch.int32: torch.full((n + GUARD,), PATTERN, dtype=torch.int32, device="cuda").view(dt)
    ws, r2c, pairs, stats = buf(need // 4), buf(P), buf(4 * P), buf(S + 1)
    coef, rw, cost = buf(P, torch.float32), buf(P, torch.float32), buf(P * nmax, torch.float32)
    near = torch.full((P * nmax + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    _lib.check(l.parq_set_match(p(lg), p(cp), I, B, Q, ncls, p(tc), p(tl), p(tn), nmax, M.COST_CLASS, M.COST_BBOX, M.RATIO, c["max_padding"],
                                seed & 0xFFFFFFFF, seed >> 32, step, p(ws), need, p(r2c), p(pairs), p(coef), p(rw), p(stats), p(cost), p(near),
                                sptr()), "parq_set_match")
    torch.cuda.synchronize()
    for t, n in ((ws, need // 4), (r2c, P), (pairs, 4 * P), (stats, S + 1), (coef, P), (rw, P), (cost, P * nmax)):
        assert (t.view(torch.int32)[n:] == PATTERN).all(), "the entry wrote behind an output"
    assert (near[P * nmax:] == 0x5A).all()
    out = dict(row_to_col=r2c[:P].view(I, B, Q), pairs=pairs[:4 * P].view(4, P), pair_coef=coef[:P], row_weight=rw[:P], stats=stats[:S + 1],
               cost=cost[:P * nmax].view(I, B, Q, nmax), near=near[:P * nmax].view(I, B, Q, nmax))
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _case(shape, variant):
    c = M.kernel_case(shape, variant)
    args = (c["logits"], c["coord"], c["t_center"], c["t_label"], c["t_count"])
    return c, M.cost_statement(*args), M.cost_statement(*args, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _run(shape, variant, seed=0x1234567887654321, step=7):
    return run_match(_case(shape, variant)[0], seed, step)


def written(c):
    """(I, B, Q, nmax) bool: the columns the entry writes."""
    return np.broadcast_to((np.arange(c["nmax"])[None, :] < c["t_count"][:, None])[None, :, None, :], (c["I"], c["B"], c["Q"], c["nmax"]))


def device_cost(c, got):
    """cost_out / near_out with the unwritten columns (still the fill pattern) set to 0 / False."""
    w = written(c)
    assert (got["cost"].view(np.int32)[~w] == PATTERN).all() and (got["near"][~w] == 0x5A).all()
    assert set(np.unique(got["near"][w]).tolist()) <= {0, 1}
    return np.where(w, got["cost"], np.float32(0)), np.where(w, got["near"], 0).astype(bool)


def assert_equals_statement(got, st, only=None):
    """Bit for bit; `only`: (I, B) bool of the segments that are compared."""
    I, B, Q = st["row_to_col"].shape
    sel = np.ones((I, B), bool) if only is None else only
    rows = np.repeat(sel.reshape(-1), Q)
    assert np.array_equal(got["row_to_col"][sel], st["row_to_col"][sel])
    assert np.array_equal(got["pairs"][:, rows], st["pairs"][:, rows])
    assert got["pair_coef"][rows].tobytes() == st["pair_coef"][rows].tobytes()
    assert got["row_weight"][rows].tobytes() == st["row_weight"][rows].tobytes()
    assert np.array_equal(got["stats"][:-1][sel.reshape(-1)], st["stats"][:-1][sel.reshape(-1)]) and got["stats"][-1] == st["stats"][-1]


@pytest.mark.parametrize("shape,variant", CASES)
def test_cost_and_near(shape, variant):
    c, (m32, near32), (m64, _) = _case(shape, variant)
    m, near = device_cost(c, _run(shape, variant))
    assert np.array_equal(near, near32)
    w = written(c)
    err = (np.abs(m.astype(np.float64) - m64) / np.maximum(1.0, np.abs(m64)))[w]
    e32 = (np.abs(m32.astype(np.float64) - m64) / np.maximum(1.0, np.abs(m64)))[w]
    print("set_match cost %-10s %-5s kernel max %.3e (%.2f x 2^-24)  numpy-float32 max %.3e" % (shape, variant, err.max(), err.max() * 2 ** 24, e32.max()))
    assert err.max() <= 32 * 2.0 ** -24


@pytest.mark.parametrize("shape,variant", CASES)
def test_matching_equals_the_statement_on_the_kernels_own_cost(shape, variant):
    c = _case(shape, variant)[0]
    got = _run(shape, variant)
    m, near = device_cost(c, got)
    st = M.match_statement(m, near, c["t_count"], 0x1234567887654321, 7, c["max_padding"])
    assert_equals_statement(got, st)
    over = M.over_full(near, c["t_count"], c["max_padding"])
    assert over.any() == (variant != "none")
    if variant == "last":
        assert (~st["punish"]).any() and (st["row_weight"] == 0).any()
    if shape == "more_boxes":
        assert (st["row_to_col"] >= 0).all()                                 # more boxes than queries: every query assigned
    again = run_match(c, 0x1234567887654321, 7)
    assert all(again[k].tobytes() == got[k].tobytes() for k in again)


@pytest.mark.parametrize("shape,variant", CASES)
def test_seed_and_step_key_the_capped_draw_only(shape, variant):
    """Another step, another low or high seed word: another draw on the over-full variants (seen in the outputs wherever the draw
    reaches them: with more boxes than queries every query keeps its assigned box), and the same bytes on the others."""
    c = _case(shape, variant)[0]
    base = _run(shape, variant)
    m, near = device_cost(c, base)
    st0 = M.match_statement(m, near, c["t_count"], 0x1234567887654321, 7, c["max_padding"])
    for seed, step in ((0x1234567887654321, 8), (0x1234567887654320, 7), (0x0234567887654321, 7)):
        got = run_match(c, seed, step)
        assert got["cost"].tobytes() == base["cost"].tobytes() and got["row_to_col"].tobytes() == base["row_to_col"].tobytes()
        st = M.match_statement(m, near, c["t_count"], seed, step, c["max_padding"])
        assert_equals_statement(got, st)
        assert np.array_equal(st["chosen"], st0["chosen"]) == (variant == "none"), (seed, step)
        same = all(got[k].tobytes() == base[k].tobytes() for k in OUT_KEYS)
        assert same == all(st[k].tobytes() == st0[k].tobytes() for k in OUT_KEYS)
        assert same or variant != "none"
        if variant != "none" and shape != "more_boxes":
            assert not same


def test_poisoned_logits_complete_with_indices_in_range():
    """NaN logits in one scene of one iteration (the outputs of a forward the range policy will re-run): the call completes, every
    index it wrote is in range or -1, the poisoned segment's cost is the stated -3.0e38f, and every segment equals the statement."""
    for shape, variant in (("odd_q", "none"), ("cfg4", "last")):
        c = _case(shape, variant)[0]
        k0, b0 = c["I"] - 1, 1
        lg = c["logits"].copy()
        lg[k0, b0] = np.nan
        lg[0, 0, 3, 1] = np.inf                                              # one row of a healthy segment
        got = run_match(c, 5, 1, logits=lg)
        m, near = device_cost(c, got)
        n = c["t_count"]
        assert (m[k0, b0, :, :n[b0]] == np.float32(-3.0e38)).all() and (m[0, 0, 3, :n[0]] == np.float32(-3.0e38)).all()
        assert np.isfinite(m).all()
        g, r2c = got["pairs"][3].reshape(c["I"], c["B"], c["Q"]), got["row_to_col"]
        for b in range(c["B"]):
            assert ((g[:, b] >= -1) & (g[:, b] < n[b])).all() and ((r2c[:, b] >= -1) & (r2c[:, b] < n[b])).all()
        assert np.isfinite(got["pair_coef"]).all() and np.isfinite(got["row_weight"]).all()
        assert_equals_statement(got, M.match_statement(m, near, n, 5, 1, c["max_padding"]))
        clean = run_match(c, 5, 1)
        others = np.ones((c["I"], c["B"]), bool)
        others[k0, b0] = others[0, 0] = False
        assert np.array_equal(got["row_to_col"][others], clean["row_to_col"][others])
        assert np.array_equal(got["near"], clean["near"])


def test_counts_outside_the_range_describe_no_boxes():
    c = dict(_case("odd_q", "none")[0])
    c["t_count"] = np.asarray([-3, 5, c["nmax"] + 1], np.int32)
    got = run_match(c, 1, 1)
    ok = c["t_count"].copy()
    ok[[0, 2]] = 0
    c["t_count"] = ok
    m, near = device_cost(c, got)
    st = M.match_statement(m, near, ok, 1, 1, c["max_padding"])
    assert_equals_statement(got, st)
    assert (got["stats"][:-1].reshape(c["I"], c["B"])[:, [0, 2]] == 0).all() and got["stats"][-1] == c["I"]
    rw = got["row_weight"].reshape(c["I"], c["B"], c["Q"])
    assert (rw[:, [0, 2]] == 0).all() and (got["pair_coef"].reshape(c["I"], c["B"], c["Q"])[:, [0, 2]] == 0).all()
    c["t_count"] = np.zeros(3, np.int32)                                      # no valid segment: all-zero constants, never 0 / 0
    got = run_match(c, 1, 1)
    assert (got["pair_coef"] == 0).all() and (got["row_weight"] == 0).all() and (got["stats"] == 0).all() and (got["pairs"][3] == -1).all()


# ---- PARQDecoder.loss with match_on_device -----------------------------------------------------------------------------------------
E2E_SEED = 4300


@functools.lru_cache(maxsize=None)
def _e2e(nbox=9, dropout=0.1):
    cfg = synth.decoder_cfg(dim=256, queries=64, heads=4, ffn=256, layers=2, dropout=dropout)
    W = synth.make_decoder_weights(cfg, E2E_SEED, damped=True)
    sc = synth.make_scene(E2E_SEED + 1, 2, 3, 32, 36, 256)
    sc_t = [dev(sc[k]) for k in ("tokens", "camera", "T_camera_pseudoCam", "T_world_pseudoCam", "T_world_local")]
    obbs, sym = synth.make_boxes(E2E_SEED + 2, 2, nbox, max_box=16)
    return cfg, W, sc_t, obbs, sym


def _step(dec, sc_t, obbs, sym, seed=5, np_seed=5):
    """One training step from fixed seeds: terms, parameter gradients, and the outputs."""
    np.random.seed(np_seed)
    torch.manual_seed(seed)                                                  # the dropout seed of the forward
    dec.zero_grad(set_to_none=True)
    outs = dec(*sc_t)
    terms = dec.loss(outs, Obb3D(dev(obbs)), Pose(sc_t[4]), dev(sym))
    terms["total_loss"].backward()
    torch.cuda.synchronize()
    return ({k: terms[k].detach().clone() for k in TERMS}, {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None},
            [{k: v.detach().clone() for k, v in o.items()} for o in outs])


def _host_packed(monkeypatch, fn, rows):
    """Runs fn() and returns its result and the packed [pairs [4][P] | coef [P] | row_weight [rows]] buffer that
    decoder_loss_batched uploaded."""
    seen, real = [], torch.from_numpy

    def spy(a):
        seen.append(np.array(a))
        return real(a)
    monkeypatch.setattr(torch, "from_numpy", spy)
    try:
        res = fn()
    finally:
        monkeypatch.undo()
    packed = [a for a in seen if a.dtype == np.int32 and a.ndim == 1 and len(a) > rows and (len(a) - rows) % 5 == 0]
    assert len(packed) == 1
    return res, packed[0]


def _targets_np(obbs, T_wl, sym):
    targets = parse_target(Obb3D(torch.from_numpy(obbs)), Pose(T_wl.cpu()))
    counts = np.asarray([len(t["labels"]) for t in targets], np.int32)
    B, nmax = len(targets), int(counts.max())
    tg = dict(t_center=np.zeros((B, nmax, 3), np.float32), t_size=np.zeros((B, nmax, 3), np.float32), t_rot=np.zeros((B, nmax, 3, 3), np.float32),
              t_label=np.zeros((B, nmax), np.int32))
    for b, t in enumerate(targets):
        n = counts[b]
        tg["t_center"][b, :n], tg["t_size"][b, :n], tg["t_label"][b, :n] = t["center"].numpy(), t["size"].numpy(), t["labels"].numpy()
        tg["t_rot"][b, :n] = t["T_rig_object"][:, :3, :3].numpy()
    return tg, counts, sym[:, :nmax].astype(np.int32)


def test_loss_with_the_matching_on_the_device_equals_the_host_matcher(monkeypatch):
    cfg, W, sc_t, obbs, sym = _e2e()
    I, B, Q = 2, 2, 64
    dec = make_decoder(cfg, W).train()
    (t_off, g_off, outs), packed = _host_packed(monkeypatch, lambda: _step(dec, sc_t, obbs, sym), I * B * Q)
    assert dec._train_pending is None and dec._match_step == 0
    dec.match_on_device = True
    t_on, g_on, _ = _step(dec, sc_t, obbs, sym, np_seed=99)
    assert dec._train_pending is None and dec._match_step == 1
    # the condition on the inputs: no cap binds, and +-1e-5 on the cost leaves scipy's assignment (tests/test_set_match_cpu.py)
    tg, counts, sym_np = _targets_np(obbs, sc_t[4], sym)
    st_np = {k: np.stack([o[k].cpu().numpy() for o in outs]) for k in outs[0]}
    m, near = M.cost_statement(st_np["pred_logits"], st_np["coord_pos"], tg["t_center"], tg["t_label"], counts)
    assert not M.over_full(near, counts, M.MAX_PADDING).any()
    from scipy.optimize import linear_sum_assignment
    rng = np.random.RandomState(1)
    for k in range(I):
        for b in range(B):
            cost = -m[k, b, :, :counts[b]].astype(np.float64)
            ref = linear_sum_assignment(cost)
            for _ in range(20):
                got = linear_sum_assignment(cost + rng.uniform(-1e-5, 1e-5, cost.shape))
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (k, b)
    # identical pairs, coefficients and row weights
    last = dec._matcher.last_device_match
    P = I * B * Q
    dp = last["packed"].cpu().numpy()
    pairs, coef, rw = dp[:4 * P].reshape(4, P), dp[4 * P:5 * P], dp[5 * P:]
    keep = pairs[3] >= 0
    Ph = (len(packed) - P) // 5
    assert Ph == keep.sum() and np.array_equal(packed[:4 * Ph].reshape(4, Ph), pairs[:, keep])
    assert np.array_equal(packed[4 * Ph:5 * Ph], coef[keep]) and np.array_equal(packed[5 * Ph:], rw)
    assert last["stats"].cpu().numpy()[-1] == I * B
    # the same step
    for k in TERMS:
        assert abs(float(t_on[k]) - float(t_off[k])) <= 1e-6 * max(1.0, abs(float(t_off[k]))), (k, float(t_on[k]), float(t_off[k]))
    assert set(g_on) == set(g_off) and len(g_on) > 20
    for n in g_on:
        den = float(g_off[n].norm())
        assert float((g_on[n] - g_off[n]).norm()) <= 1e-4 * max(den, 1e-6), n     # float atomics in the backward: not bit-identical
    # terms and output gradients against the float64 oracle on the device's pairs (the outputs as leaves: not a forward in flight)
    leaves = [{k: v.clone().requires_grad_(k != "coord_pos") for k, v in o.items()} for o in outs]
    terms = dec.loss(leaves, Obb3D(dev(obbs)), Pose(sc_t[4]), dev(sym))
    assert dec._match_step == 2
    terms["total_loss"].backward()
    dp = dec._matcher.last_device_match["packed"].cpu().numpy()
    pairs, coef, rw = dp[:4 * P].reshape(4, P), dp[4 * P:5 * P], dp[5 * P:]
    assert np.array_equal(packed[:4 * Ph].reshape(4, Ph), pairs[:, pairs[3] >= 0])
    names = {"logits": "pred_logits", "center": "center_unnormalized", "size": "size_unnormalized", "o6": "ortho6d"}
    outputs = {s: st_np[l] for s, l in names.items()}
    cw = np.ones(10, np.float32)
    cw[9] = 0.1
    args = (outputs, tg, pairs, coef.view(np.float32), rw.view(np.float32), cw, dec.loss_weight, sym_np)
    r64, r32 = set_loss_oracle(*args, dtype=torch.float64), set_loss_oracle(*args, dtype=torch.float32)
    got_terms = np.asarray([float(terms[k].detach()) for k in TERMS[:4]])
    got_grads = [torch.stack([o[names[s]].grad for o in leaves]).cpu().numpy() for s in ("logits", "center", "size", "o6")]
    compare("device matching", got_terms, got_grads, r64, r32, rot_rows_left_out(dict(outputs=outputs, pairs=pairs), r64))


@pytest.fixture
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev)


def test_capped_draw_does_not_depend_on_numpy_random(deterministic):
    """A neighbourhood of L1 < 3 puts most reference points near every box: the cap binds everywhere.  With the matching on the device
    two steps under different np.random states give the same bits; another match_seed gives another step."""
    cfg, W, sc_t, obbs, sym = _e2e()
    dec = make_decoder(cfg, W).train()
    dec.match_on_device = True
    dec._matcher = HungarianMatcherModified(cost_class=2, cost_bbox=0.25, ratio=3.0)
    dec._class_weight = torch.ones(10)
    dec._class_weight[9] = 0.1
    runs = []
    for np_seed, match_seed in ((1, 0), (2, 0), (1, 77)):
        dec._match_step, dec.match_seed = 0, match_seed
        runs.append(_step(dec, sc_t, obbs, sym, np_seed=np_seed))
        assert dec._match_step == 1
    (ta, ga, outs), (tb, gb, _), (tc, gc, _) = runs
    tg, counts, _ = _targets_np(obbs, sc_t[4], sym)
    m, near = M.cost_statement(np.stack([o["pred_logits"].cpu().numpy() for o in outs]), np.stack([o["coord_pos"].cpu().numpy() for o in outs]),
                               tg["t_center"], tg["t_label"], counts, ratio=3.0)
    assert M.over_full(near, counts, M.MAX_PADDING).sum() >= 4                # the cap binds
    assert all(torch.equal(ta[k], tb[k]) for k in TERMS) and set(ga) == set(gb) and all(torch.equal(ga[n], gb[n]) for n in ga)
    assert not torch.equal(ta["total_loss"], tc["total_loss"])


def test_poisoned_forward_is_rerun_behind_the_enqueued_matching():
    """Tokens that leave the fp16 range: the forward's outputs are NaN when matching and loss are enqueued behind it.  The one wait of
    loss() finds the flag, the forward is re-run with the exact fp32 kernels and matching and loss are enqueued again with the same
    step: finite terms and gradients, as with the host matcher (tests/test_gpu_loss.py)."""
    import warnings
    cfg = synth.decoder_cfg(dim=256, queries=32, heads=4, ffn=128, layers=2, dropout=0.0)
    W = synth.make_decoder_weights(cfg, 821, damped=True)
    sc = synth.make_scene(822, 1, 2, 32, 36, 256)
    sc["tokens"] = (sc["tokens"] * np.float32(2e4)).astype(np.float32)
    sc_t = [dev(sc[k]) for k in ("tokens", "camera", "T_camera_pseudoCam", "T_world_pseudoCam", "T_world_local")]
    obbs, sym = synth.make_boxes(823, 1, 6)
    res = {}
    for on in (False, True):
        dec = make_decoder(cfg, W).train()
        dec.match_on_device = on
        assert dec._train_mode() == "split" and dec.overlap_loss_matching
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            res[on] = _step(dec, sc_t, obbs, sym, seed=7)
        assert any("fp16 range" in str(r.message) for r in rec)
        assert dec.attention_mode == "fp32" and dec._train_pending is None and dec._match_step == int(on)
        assert all(bool(torch.isfinite(v)) for v in res[on][0].values()) and all(torch.isfinite(g).all() for g in res[on][1].values())
    stats = dec._matcher.last_device_match["stats"].cpu().numpy()
    assert stats[-1] == 2 and (stats[:-1] >= 6).all()


def test_empty_scene_and_fp16_outputs_take_the_host_path():
    cfg, W, sc_t, obbs, sym = _e2e()
    dec = make_decoder(cfg, W)
    with torch.no_grad():
        outs = [{k: v.clone() for k, v in o.items()} for o in dec(*sc_t)]
    torch.cuda.synchronize()
    empty = obbs.copy()
    empty[1] = -1.0
    for tag, o, ob in (("empty scene", outs, empty), ("fp16", [{k: v.half() for k, v in d.items()} for d in outs], obbs)):
        res = {}
        for on in (False, True):
            dec.match_on_device = on
            dec._match_step = 0
            np.random.seed(3)
            try:
                res[on] = dec.loss(o, Obb3D(dev(ob)), Pose(sc_t[4]), dev(sym))
            except RuntimeError as e:                                        # whatever the host path does with such outputs, both do
                res[on] = type(e)
            assert dec._match_step == 0, tag                                  # the host path was taken
        if isinstance(res[False], dict):
            assert all(torch.equal(res[True][k], res[False][k]) for k in TERMS), tag
        else:
            assert res[True] is res[False] and tag == "fp16", tag
    dec.match_on_device = True
    dec.loss(outs, Obb3D(dev(obbs)), Pose(sc_t[4]), dev(sym))
    assert dec._match_step == 1


def test_device_matching_reproduces_golden_g10():
    """g10's matching draws no random number (tests/test_set_match_cpu.py), so the device path is held to the reference's terms at the
    tolerance of tests/test_gpu_loss.py."""
    c = LOSS_CASE
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "g10_loss.npz"))
    assert json.loads(bytes(z["meta"]).decode()) == json.loads(json.dumps(c))
    outs, obbs, T_wl, sym = loss_case_inputs(c)
    cfg = synth.decoder_cfg(dim=64, queries=c["Q"], heads=1, ffn=64, layers=c["I"])
    from parq_amd.decoder import PARQDecoder
    dec = PARQDecoder(cfg).cuda()
    dec.match_on_device = True
    touts = [{k: torch.from_numpy(v).cuda() for k, v in o.items()} for o in outs]
    got = dec.loss(touts, Obb3D(torch.from_numpy(obbs).cuda()), Pose(torch.from_numpy(T_wl).cuda()), torch.from_numpy(sym).cuda())
    assert dec._match_step == 1
    for k in TERMS:
        want = float(z["sym_%s" % k])
        assert abs(float(got[k]) - want) < 2e-5 * max(1.0, abs(want)), (k, float(got[k]), want)
    assert dec._matcher.last_device_match["stats"].cpu().numpy()[-1] == c["I"] * c["B"]
